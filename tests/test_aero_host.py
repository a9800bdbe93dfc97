"""CPU check of the device aero-servo matrices (raft-teststuff_amd/csrc/rh_aero.h) against the Python
they restate (Rotor.calcAero, FOWT.calcTurbineConstants, prep.linear_matrices): the header is
compiled for the host with g++ (tools/aero_host.cpp), so the same coefficient, pattern, mean-load
and summing code the GPU runs is compared here without a GPU.  Also the ABI entry's validation, the
Python surface's refusals and the new keyword of analyzeCasesBatch."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import load_design

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import aero_cases as AC  # noqa: E402

# The worst difference of sum_r A_aero, sum_r B_aero and f_aero0 between the host-compiled header and
# the Python over the 20 cases of test_aero_term_alone (aeroServoMod 1 and 2, five speeds, two
# headings), measured on the CPU, per case and normwise over all bins relative to the largest entry
# of that case's term, on the design's 40 bins: 1.65e-15 (sum_r B_aero; sum_r A_aero 5.69e-16, f_aero0
# 2.80e-16: a few roundings per entry, since the Python scales R diag(a, 0, 0) R^T per bin and
# translates it while the header translates the pattern once and scales it).  The gyroscopic matrix
# agrees bit for bit.  The tests assert at ten times that, and never above 1e-10.
AERO_TERM_MEASURED = 1.65e-15
AERO_TERM_BAR = min(10 * AERO_TERM_MEASURED, 1e-10)
CONDITION_MAX = 1e3


@pytest.fixture(scope="module")
def lib():
    return AC.host_lib()


@pytest.fixture(scope="module")
def cases():
    """mod -> (fowt, [(case, pair inputs, Python terms)]) for the five speeds and two headings: computed once."""
    out = {}
    for mod in (1, 2):
        m = AC.posed_model(mod)
        fowt = m.fowtList[0]
        rows = []
        for h in AC.HEADINGS:
            for U in AC.SPEEDS:
                case = AC.wind_case(U, h)
                pin = AC.pair_inputs(fowt, case)
                rows.append((case, pin, AC.python_terms(fowt, case, [pin["bem"]])))
        out[mod] = (fowt, rows)
    return out


def _zeroed_gyro(param):
    from raft import _native as N
    p = np.array(param)
    p[..., N.AP["GYRO"]:N.AP["GYRO"] + 3] = 0.0
    return p


# ------------------------------------------------------------------------------ the aero term alone
def test_denominator_is_well_conditioned(cases):
    """Asserted from the Python alone: over the tested bins the sum of the magnitudes of the terms of
    H_QT's denominator stays below 1e3 times the magnitude of the denominator at every tested speed,
    so a bar near rounding level means something (no speed had to be replaced)."""
    fowt, rows = cases[2]
    worst = 0.0
    for case, pin, _ in rows:
        worst = max(worst, AC.denominator_condition(fowt.rnaList[0], pin["dloads"], pin["param"], fowt.w))
    print(f"denominator condition: {worst:.3g}")
    assert worst < CONDITION_MAX, worst


def test_denominator_matches_python(lib, cases):
    """The header's denominator against rotor.py's expression, relative to its magnitude."""
    from raft import _native as N
    from raft.rotor import RAD2DEG, RPM2RADPS
    fowt, rows = cases[2]
    rot, w = fowt.rnaList[0], np.ascontiguousarray(fowt.w, dtype=float)
    for case, pin, _ in rows:
        par, D = np.ascontiguousarray(pin["param"]), np.ascontiguousarray(pin["dloads"])
        dQ_dOm, dQ_dPi = D[4] / RPM2RADPS, D[5] * RAD2DEG
        ref = rot.I_drivetrain * w ** 2 + (dQ_dOm + par[N.AP["KP_BETA"]] * dQ_dPi - rot.Ng * par[N.AP["KP_TAU"]]) * 1j * w \
            + par[N.AP["KI_BETA"]] * dQ_dPi - rot.Ng * par[N.AP["KI_TAU"]]
        re, im = np.zeros(len(w)), np.zeros(len(w))
        lib.rh_aero_denominator_host(par.ctypes.data, D.ctypes.data, len(w), w.ctypes.data, re.ctypes.data, im.ctypes.data)
        assert np.max(np.abs((re + 1j * im) - ref) / np.abs(ref)) <= AERO_TERM_BAR


@pytest.mark.parametrize("mod", [1, 2])
def test_aero_term_alone(lib, cases, mod):
    """sum_r A_aero, sum_r B_aero, the alternator part and f_aero0 of the host-compiled header with
    M0 = B0 = 0 against the Python, per case."""
    from raft import _native as N
    fowt, rows = cases[mod]
    w = np.asarray(fowt.w, dtype=float)
    Z = np.zeros([6, 6])
    worst = 0.0
    gates = set()
    for case, pin, ref in rows:
        assert pin["mode"] == mod
        args = ([0], [pin["mode"]], pin["loads"][None], pin["dloads"][None])
        M, B, f0 = AC.host_mb(lib, 1, *args, _zeroed_gyro(pin["param"])[None], w, Z, Z)
        errs = dict(A=AC.term_error(M[0], ref["A"]), B=AC.term_error(B[0], ref["B"]), f0=AC.term_error(f0[0], ref["f0"]))
        worst = max(worst, *errs.values())
        assert max(errs.values()) <= AERO_TERM_BAR, (case["wind_speed"], case["wind_heading"], errs)
        G = np.zeros(36)
        g = np.ascontiguousarray(pin["param"][N.AP["GYRO"]:N.AP["GYRO"] + 3])
        lib.rh_aero_gyro_host(g.ctypes.data, G.ctypes.data)
        assert np.array_equal(G.reshape(6, 6), ref["G"]) and np.any(ref["G"])
        # with the gyroscopic vector, B gains exactly that matrix on top
        _, B2, _ = AC.host_mb(lib, 1, *args, pin["param"][None], w, Z, Z)
        assert np.array_equal(B2[0], B[0] + ref["G"])
        assert np.any(ref["B"]) and bool(np.any(ref["A"])) == (mod == 2)
        gates.add((pin["param"][N.AP["KP_BETA"]] == 0, pin["param"][N.AP["KP_TAU"]] == 0))
    print(f"aeroServoMod {mod}: worst term difference {worst:.3e}")
    assert gates == {(True, False), (False, True)}     # below rated the torque gains are live, above the pitch gains


def test_two_pairs_on_one_case(lib):
    """Two pairs of different q, r_hub_rel and mode on case 2 of three, a pair on case 0, none on
    case 1: case 2 equals the sum of the two single-pair results, case 1 the base bit for bit."""
    loads, dloads, param, modes = AC.synthetic_pairs()
    rng = np.random.default_rng(7)
    w = np.linspace(0.05, 2.0, 37)
    for M0 in (rng.normal(size=[6, 6]) * 1e7, rng.normal(size=[37, 6, 6]) * 1e7):
        B0 = -0.5 * M0
        M, B, f0 = AC.host_mb(lib, 3, [0, 2, 2], [modes[1], *modes], loads[[1, 0, 1]], dloads[[1, 0, 1]], param[[1, 0, 1]],
                              w, M0, B0)
        assert np.array_equal(M[1], np.broadcast_to(M0, [37, 6, 6])) and np.array_equal(B[1], np.broadcast_to(B0, [37, 6, 6]))
        assert not np.any(f0[1])
        Z = np.zeros_like(M0)
        single = [AC.host_mb(lib, 1, [0], [modes[p]], loads[[p]], dloads[[p]], param[[p]], w, Z, Z) for p in (0, 1)]
        both = AC.host_mb(lib, 1, [0, 0], modes, loads, dloads, param, w, Z, Z)
        for k in range(3):
            assert AC.term_error(both[k][0], single[0][k][0] + single[1][k][0]) <= AERO_TERM_BAR
        assert np.any(single[0][0]) and not np.any(single[1][0])       # mode 2 has added mass, mode 1 none
        # ... and with the base: case 2 is the pairs' sum plus the base, case 0 the second pair alone plus the base
        assert np.allclose(M[2], both[0][0] + M0, rtol=0, atol=8 * AC.EPS * np.abs(M[2]).max())
        assert np.allclose(B[0], single[1][1][0] + B0, rtol=0, atol=8 * AC.EPS * np.abs(B[0]).max())
        assert np.array_equal(f0[2], both[2][0]) and np.array_equal(f0[0], single[1][2][0])


@pytest.mark.parametrize("per_bin", [False, True], ids=["constant", "per_bin"])
@pytest.mark.parametrize("mod", [1, 2])
def test_with_the_real_base(lib, mod, per_bin):
    """M and B with the design's own base against prep.linear_matrices, per bin within
    8 eps max|entry| of that bin's matrix.  The bound is derived: the two sides add the same four terms
    in a different association, each of the at most three roundings that differ is at most eps / 2 of
    a partial sum no larger than the largest entry, and 8 leaves a factor of five.  per_bin: a seeded
    A_BEM / B_BEM on the FOWT, so that M0 and B0 are [nw, 6, 6]."""
    fowt = AC.posed_model(mod).fowtList[0]
    if per_bin:
        rng = np.random.default_rng(11)
        fowt.A_BEM = rng.normal(size=[6, 6, fowt.nw]) * 1e6
        fowt.B_BEM = rng.normal(size=[6, 6, fowt.nw]) * 1e5
    w = np.asarray(fowt.w, dtype=float)
    worst = 0.0
    for U, h in ((8, 20.0), (14, 0.0)):
        case = AC.wind_case(U, h)
        M0, B0 = AC.base_matrices(fowt, case)
        assert M0.shape == ((fowt.nw, 6, 6) if per_bin else (6, 6))
        pin = AC.pair_inputs(fowt, case)
        ref = AC.python_terms(fowt, case, [pin["bem"]])
        M, B, _ = AC.host_mb(lib, 1, [0], [pin["mode"]], pin["loads"][None], pin["dloads"][None], pin["param"][None], w, M0, B0)
        for got, want in ((M[0], ref["M_lin"]), (B[0], ref["B_lin"])):
            for i in range(fowt.nw):
                bound = 8 * AC.EPS * np.abs(want[i]).max()
                if bound > 0:
                    worst = max(worst, np.abs(got[i] - want[i]).max() / bound)
                assert np.abs(got[i] - want[i]).max() <= bound, (U, h, i, np.abs(got[i] - want[i]).max(), bound)
    print(f"aeroServoMod {mod}, per_bin {per_bin}: largest difference / bound {worst:.2f}")


def test_stand_alone_program_runs():
    """tools/aero_host.cpp's own main (both modes, a case without a pair, two pairs on one case, a
    refused table) under the address and undefined-behaviour sanitizers."""
    import tempfile
    exe = os.path.join(tempfile.mkdtemp(), "aero_host")
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                    "-DAERO_HOST_MAIN", "-o", exe, os.path.join(AC.ROOT, "tools", "aero_host.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "0 failures" in out.stdout, out.stdout + out.stderr


# ------------------------------------------------------------------------------ ABI
@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as g
    g.build()
    from raft import _native as N
    return N, N.lib()


def _abi_args(N, ncase=2, npair=2, nw=3, pair_case=(0, 1), modes=(1, 2), ctx=True):
    """Host buffers standing in for every pointer: the entry validates before it touches any of them
    (and before it reads the context), so no device is needed to see a refusal."""
    keep = dict(ctx=ctypes.create_string_buffer(4096), pc=np.array(pair_case, dtype=np.int32),
                md=np.array(modes, dtype=np.int32), buf=np.zeros(4096))
    b = keep["buf"].ctypes.data
    args = [ctypes.addressof(keep["ctx"]) if ctx else None, ncase, npair, nw, b, b, keep["pc"].ctypes.data,
            keep["md"].ctypes.data, b, b, b, b, b, 0, b, b, b, None]
    return args, keep


def test_symbol_and_version(native):
    N, L = native
    assert hasattr(L, "rh_rotor_aero_mb")
    assert L.rh_version() == 8
    src = open(os.path.join(AC.ROOT, "include", "rafthip.h")).read()
    assert f"RH_AP_COUNT = {N.AP_COUNT}" in src and f"#define RH_AERO_MAX_PAIRS {N.AERO_MAX_PAIRS}" in src
    for name in ("MODE", "RQ", "RHUB", "I_DRIVETRAIN", "GYRO"):       # the entries the header numbers itself
        assert f"RH_AP_{name} = {N.AP[name]}" in src
    run = ("I_DRIVETRAIN", "NG", "K_FLOAT", "KP_BETA", "KI_BETA", "KP_TAU", "KI_TAU")   # ... and the run that follows on
    assert [N.AP[k] for k in run] == list(range(13, 20))
    assert src.index("RH_AP_NG") < src.index("RH_AP_K_FLOAT") < src.index("RH_AP_KP_BETA") < src.index("RH_AP_KI_BETA") \
        < src.index("RH_AP_KP_TAU") < src.index("RH_AP_KI_TAU") < src.index("RH_AP_GYRO")


def test_entry_refuses_bad_arguments(native):
    N, L = native
    args, keep = _abi_args(N, ctx=False)
    assert L.rh_rotor_aero_mb(*args) == N.RH_EINVAL and b"null context" in L.rh_last_error()
    for k, what in ((1, "ncase"), (2, "npair"), (3, "nw")):
        args, keep = _abi_args(N)
        args[k] = 0
        assert L.rh_rotor_aero_mb(*args) == N.RH_EINVAL and what.encode() in L.rh_last_error()
    for k in (4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 15, 16):
        args, keep = _abi_args(N)
        args[k] = None
        assert L.rh_rotor_aero_mb(*args) == N.RH_EINVAL and b"null" in L.rh_last_error(), k
    args, keep = _abi_args(N, pair_case=(1, 0))
    assert L.rh_rotor_aero_mb(*args) == N.RH_EINVAL and b"decreases" in L.rh_last_error()
    args, keep = _abi_args(N, pair_case=(0, 2))
    assert L.rh_rotor_aero_mb(*args) == N.RH_EINVAL and b"outside [0, 2)" in L.rh_last_error()
    args, keep = _abi_args(N, pair_case=(-1, 0))
    assert L.rh_rotor_aero_mb(*args) == N.RH_EINVAL and b"outside [0, 2)" in L.rh_last_error()
    args, keep = _abi_args(N, modes=(1, 3))
    assert L.rh_rotor_aero_mb(*args) == N.RH_EINVAL and b"aeroServoMod 3" in L.rh_last_error()
    args, keep = _abi_args(N, ncase=1, npair=9, pair_case=(0,) * 9, modes=(1,) * 9)
    assert L.rh_rotor_aero_mb(*args) == N.RH_EINVAL and b"more than 8 pairs" in L.rh_last_error()
    args, keep = _abi_args(N)
    args[14] += 8
    assert L.rh_rotor_aero_mb(*args) == N.RH_EINVAL and b"16-byte aligned" in L.rh_last_error()


# ------------------------------------------------------------------------------ Python surface
WIND = AC.wind_case(10.0, 0.0)


def _no_device(monkeypatch):
    """Any device call from here on fails the test: a context, or a tensor made for DeviceRotor's tables
    (DeviceRotor.__init__ flattens, and so refuses, before it makes the first)."""
    import torch
    from raft import _native as N

    def boom(*a, **k):
        raise AssertionError("a device call before the refusal")
    monkeypatch.setattr(N, "context", boom)
    for name in ("tensor", "empty", "device"):
        monkeypatch.setattr(torch, name, boom)


def test_analyze_cases_batch_refusals():
    import raft
    m = raft.Model(load_design("VolturnUS-S_aero"))
    with pytest.raises(NotImplementedError, match="aero_device=True with statics=True"):
        m.analyzeCasesBatch([dict(WIND)], aero_device=True, statics=True)
    farm = raft.Model(load_design("VolturnUS-S_farm_aero"))
    assert farm.nFOWT > 1
    with pytest.raises(NotImplementedError, match="aero_device=True on an array"):
        farm.analyzeCasesBatch([dict(WIND)], aero_device=True)


def test_aero_mb_batch_refusals_come_before_any_device_call(monkeypatch):
    import raft
    import raft.ccblade as C
    _no_device(monkeypatch)
    fowt = raft.Model(load_design("VolturnUS-S_aero")).fowtList[0]
    rot = fowt.rnaList[0]
    assert fowt.aeroMBBatch([dict(WIND, turbine_status="parked"), dict(WIND, wind_speed=0.0)], None) is None
    rot.aeroServoMod = 3
    with pytest.raises(NotImplementedError, match="aeroServoMod = 3"):
        fowt.aeroMBBatch([dict(WIND)], None)
    rot.aeroServoMod = 2
    rot.ccblade.iterRe = 2
    with pytest.raises(NotImplementedError, match="iterRe = 2"):
        fowt.aeroMBBatch([dict(WIND)], None)
    rot.ccblade.iterRe = 1
    real, rot.ccblade = rot.ccblade, object()
    with pytest.raises(NotImplementedError, match="not the restatement class"):
        fowt.aeroMBBatch([dict(WIND)], None)
    rot.ccblade = real
    fowt._rotor_submerged = True
    with pytest.raises(NotImplementedError, match="underwater rotors"):
        fowt.aeroMBBatch([dict(WIND)], None)
    assert C.CCBlade is type(real)


def test_rotor_loads_batch_shares_the_operating_points():
    """The shared steps give rotorLoadsBatch's pairs and operating points: the pairs in case and rotor
    order, each point as Rotor.operating_point and inflow_angles form it."""
    import raft
    fowt = raft.Model(load_design("VolturnUS-S_aero")).fowtList[0]
    cs = [dict(WIND), dict(WIND, turbine_status="parked"), dict(WIND, wind_speed=14.0, wind_heading=20.0)]
    pairs, rotors = fowt._rotor_pairs(cs)
    assert pairs == [(0, 0), (2, 0)] and rotors == [0]
    seen = []
    op, idx = fowt._rotor_operating_points(pairs, rotors, cs, each=lambda n, rot, speed: seen.append((n, speed, rot.yaw)))
    rot = fowt.rnaList[0]
    for n, (ic, _) in enumerate(pairs):
        want = (*rot.operating_point(cs[ic]["wind_speed"]), *rot.inflow_angles(cs[ic]))
        assert np.array_equal(op[n], want) and seen[n][:2] == (n, cs[ic]["wind_speed"]) and seen[n][2] == rot.yaw
    assert list(idx) == [0, 0]

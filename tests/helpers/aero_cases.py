"""Shared by tests/test_aero_host.py and tests/test_gpu_aero_mb.py: the host build of csrc/rh_aero.h
(tools/aero_host.cpp), the wind cases of the aero-servo matrix checks, the inputs of one (case,
rotor) pair as the device path forms them, and the Python reference values (FOWT.calcTurbineConstants
with bem= that pair, then prep.linear_matrices), computed once per module and kept unchanged."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SPEEDS = [4, 8, 10.59, 14, 24]          # the schedule speeds: both sides of rated
HEADINGS = [0.0, 20.0]                   # wind headings [deg]
POSE = [2.0, 1.0, -0.5, 0.02, 0.06, 0.15]   # a yawed, pitched platform: R_q and r_hub_rel are full
EPS = np.finfo(float).eps

_p, _i = ctypes.c_void_p, ctypes.c_int


def host_lib():
    """tools/aero_host.cpp compiled with g++ (no fused multiply-add, as the device build)."""
    out = os.path.join(tempfile.mkdtemp(), "aero_host.so")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", out,
                    os.path.join(ROOT, "tools", "aero_host.cpp")], check=True)
    L = ctypes.CDLL(out)
    L.rh_aero_pair_host.argtypes = [_p, _p, _i, _p, _p, _p, _p]
    L.rh_aero_denominator_host.argtypes = [_p, _p, _i, _p, _p, _p]
    L.rh_aero_gyro_host.argtypes = [_p, _p]
    for f in (L.rh_aero_pair_host, L.rh_aero_denominator_host, L.rh_aero_gyro_host):
        f.restype = None
    L.rh_rotor_aero_mb_host.argtypes = [_i, _i, _i, _p, _p, _p, _p, _p, _p, _p, _p, _i, _p, _p, _p]
    L.rh_rotor_aero_mb_host.restype = _i
    return L


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def host_mb(L, ncase, pair_case, modes, loads, dloads, param, w, M0, B0):
    """rh_rotor_aero_mb_host: M [ncase, nw, 6, 6], B and f_aero0 [ncase, 6] of the host-compiled header."""
    pc, md = np.ascontiguousarray(pair_case, dtype=np.int32), np.ascontiguousarray(modes, dtype=np.int32)
    loads, dloads, param, w, M0, B0 = (_f64(a) for a in (loads, dloads, param, w, M0, B0))
    nw = len(w)
    M, B, f0 = np.zeros([ncase, nw, 6, 6]), np.zeros([ncase, nw, 6, 6]), np.zeros([ncase, 6])
    rc = L.rh_rotor_aero_mb_host(ncase, len(pc), nw, w.ctypes.data, pc.ctypes.data, md.ctypes.data, loads.ctypes.data,
                                 dloads.ctypes.data, param.ctypes.data, M0.ctypes.data, B0.ctypes.data,
                                 int(M0.ndim == 3), M.ctypes.data, B.ctypes.data, f0.ctypes.data)
    assert rc == 0, rc
    return M, B, f0


def wind_case(speed, heading):
    return {"wind_speed": float(speed), "wind_heading": float(heading), "turbulence": 0.1, "turbine_status": "operating",
            "yaw_misalign": 0, "wave_spectrum": "JONSWAP", "wave_period": 10, "wave_height": 4, "wave_heading": 0,
            "current_speed": 0, "current_heading": 0}


def posed_model(mod, settings=None):
    """VolturnUS-S_aero with aeroServoMod = mod, the platform at POSE."""
    import raft
    from conftest import load_design
    d = load_design("VolturnUS-S_aero")
    d["turbine"]["aeroServoMod"] = mod
    if settings:
        d.setdefault("settings", {}).update(settings)
    m = raft.Model(d)
    m.fowtList[0].setPosition(POSE)
    return m


def pair_inputs(fowt, case, ir=0):
    """One (case, rotor) pair as FOWT.aeroMBBatch forms it, with the blade-element solve of
    raft.ccblade on the host: loads [8], dloads [6], the parameter row, the mode, and the `bem`
    entry that gives FOWT.calcTurbineConstants the same loads."""
    from raft.rotor_device import aero_mode, aero_param_row
    rot = fowt.rnaList[ir]
    speed = float(case["wind_speed"])
    tilt, yaw = rot.inflow_angles(case)
    Uhub, Om, pit = rot.operating_point(speed)
    rot.ccblade.tilt, rot.ccblade.yaw = tilt, yaw
    loads, derivs = rot.ccblade.evaluate(Uhub, Om, pit, coefficients=True)
    L8 = np.array([loads[k][0] for k in ("T", "Y", "Z", "Q", "My", "Mz", "Mb", "P")])
    D6 = np.array([derivs[a][b][0, 0] for a in ("dT", "dQ") for b in ("dUinf", "dOmega", "dpitch")])
    mode = aero_mode(rot, ir)
    return dict(loads=L8, dloads=D6, param=aero_param_row(rot, speed, mode), mode=mode, bem=(loads, derivs))


def python_terms(fowt, case, bem):
    """The Python's terms of one case: sum_r A_aero and sum_r B_aero [nw, 6, 6], the summed B_gyro
    [6, 6], the summed f_aero0 [6], and M, B of prep.linear_matrices [nw, 6, 6] (constant ones tiled)."""
    from raft.prep import linear_matrices
    fowt.calcTurbineConstants(dict(case), ptfm_pitch=0, bem=bem)
    A = np.moveaxis(np.sum(fowt.A_aero, axis=3), 2, 0).copy()
    B = np.moveaxis(np.sum(fowt.B_aero, axis=3), 2, 0).copy()
    M_lin, B_lin, _, per_bin = linear_matrices(fowt)
    if not per_bin:
        M_lin, B_lin = np.tile(M_lin, (fowt.nw, 1, 1)), np.tile(B_lin, (fowt.nw, 1, 1))
    return dict(A=A, B=B, G=np.sum(fowt.B_gyro, axis=2), f0=np.sum(fowt.f_aero0, axis=1), M_lin=M_lin, B_lin=B_lin)


def base_matrices(fowt, case):
    """M0, B0 of the aero-free design (what the DeviceDesign of analyzeCasesBatch's base holds)."""
    from raft.prep import linear_matrices
    fowt.calcTurbineConstants(dict(case, wind_speed=0.0), ptfm_pitch=0)
    M0, B0, _, _ = linear_matrices(fowt)
    return np.array(M0), np.array(B0)


def denominator_condition(rot, D6, param, w):
    """From the Python alone: over the bins, the largest sum of the magnitudes of the terms of H_QT's
    denominator divided by the magnitude of the denominator."""
    from raft import _native as N
    from raft.rotor import RAD2DEG, RPM2RADPS
    dQ_dOm, dQ_dPi = D6[4] / RPM2RADPS, D6[5] * RAD2DEG
    kpb, kib = param[N.AP["KP_BETA"]], param[N.AP["KI_BETA"]]
    kpt, kit = param[N.AP["KP_TAU"]], param[N.AP["KI_TAU"]]
    terms = [rot.I_drivetrain * w ** 2, dQ_dOm * 1j * w, kpb * dQ_dPi * 1j * w, -rot.Ng * kpt * 1j * w,
             kib * dQ_dPi + 0 * w, -rot.Ng * kit + 0 * w]
    return float(np.max(sum(np.abs(t) for t in terms) / np.abs(sum(terms))))


def term_error(got, ref):
    """Normwise difference over all bins relative to the largest entry of the reference term."""
    scale = np.abs(ref).max()
    if scale == 0.0:
        assert not np.any(got)
        return 0.0
    return float(np.linalg.norm(np.asarray(got) - ref) / scale)


def synthetic_pairs():
    """Two pairs of different q, r_hub_rel and mode for one case, at the ABI level (no golden design
    has two rotors): loads [2, 8], dloads [2, 6], param [2, AP_COUNT], modes."""
    from raft import _native as N
    from raft.hydro_math import rotation_matrix
    loads = np.array([[1.5e6, 2e3, -1e4, 1.9e7, 4e5, -2e5, 3e7, 1.5e7], [0.9e6, -5e3, 3e4, 1.1e7, -2e5, 6e5, 2e7, 0.8e7]])
    dloads = np.array([[2.1e5, 1.6e5, -1.2e5, 1.5e6, -3.4e6, -1.9e6], [1.3e5, 2.2e5, -0.7e5, 0.8e6, -2.1e6, -2.6e6]])
    param = np.zeros([2, N.AP_COUNT])
    for p, (mode, ang, r) in enumerate([(2, (0.0, 0.1, 0.3), (-10.0, 40.0, 150.0)), (1, (0.02, 0.05, -0.4), (-12.0, -40.0, 140.0))]):
        R = rotation_matrix(*ang)
        param[p, N.AP["MODE"]] = mode
        param[p, N.AP["RQ"]:N.AP["RQ"] + 9] = R.reshape(9)
        param[p, N.AP["RHUB"]:N.AP["RHUB"] + 3] = r
        param[p, N.AP["I_DRIVETRAIN"]], param[p, N.AP["NG"]], param[p, N.AP["K_FLOAT"]] = 3.2e8, 1.0, -9.0
        param[p, N.AP["KP_BETA"]], param[p, N.AP["KI_BETA"]] = 0.6 + 0.1 * p, 0.1
        param[p, N.AP["GYRO"]:N.AP["GYRO"] + 3] = 2.5e8 * R[:, 0] * (1 + p)
    return loads, dloads, param, [2, 1]

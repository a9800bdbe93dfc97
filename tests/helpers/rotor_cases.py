"""Shared by tests/test_rotor_host.py and tests/test_gpu_rotor.py: the operating points of the
rotor parity checks, the Python reference values of raft/ccblade.py (computed once per rotor and
kept unchanged), the self-calibrated derivative bars, and the host build of csrc/rh_rotor.h."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (Uinf [m/s], Omega [rpm], pitch [deg]) -- the branches each reaches were checked with the Python
POINTS = [(8, 5.6, 0),                                    # first bracket; four sections past a = 0.4
          (3, 7.5, 0), (4, 9, -2),                        # most sections in Buhl's region; negative torque
          (25, 3, 0), (12, 0.5, 0),                       # one to three sections in the third bracket
          (25, 7.5, 40), (10, 7.5, 30), (6, 7.5, 20),     # negative thrust
          (2, 9, 5),
          (10, 0, 0)]                                     # not rotating
SECOND_BRACKET_POINTS = [(15, 0.5, 90), (8, -5, 0)]      # found by a search on the CPU (test_rotor_host.py)
SCHEDULE_U = [4, 8, 10.59, 14, 24]                        # the derivative checks: on the operating schedule
PHI_TOL = 1e-11      # 2.5 x 2 (xtol + rtol |phi|): two solvers that each meet brentq's contract
LOAD_TOL = 1e-9      # of |T| (forces) and |Q| (moments): ten times the effect of phi moved by 4e-12
KEYS = ("T", "Y", "Z", "Q", "My", "Mz", "Mb", "P")

_d, _p, _i = ctypes.c_double, ctypes.c_void_p, ctypes.c_int


def host_lib():
    """tools/rotor_host.cpp compiled with g++ (no fused multiply-add, as the device build)."""
    out = os.path.join(tempfile.mkdtemp(), "rotor_host.so")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", out,
                    os.path.join(ROOT, "tools", "rotor_host.cpp")], check=True)
    L = ctypes.CDLL(out)
    L.rh_rotor_spline_host.argtypes = [_i, _i, _p, _p, _p, _i, _p, _p, _p]
    L.rh_rotor_relative_wind_host.argtypes = [_d] * 10 + [_p]
    L.rh_rotor_induction_host.argtypes = [_d] * 7 + [_i, _d, _d, _i, _p]
    L.rh_rotor_section_eval_host.argtypes = [_p, _i, _d, _i, _d, _d, _d, _p]
    L.rh_rotor_section_solve_host.argtypes = [_p, _i, _p, _d, _i, _p]
    L.rh_rotor_loads_host.argtypes = [_p, _i, _p, _p, _p, _p, _p]
    for f in (L.rh_rotor_spline_host, L.rh_rotor_relative_wind_host, L.rh_rotor_induction_host,
              L.rh_rotor_section_eval_host, L.rh_rotor_section_solve_host, L.rh_rotor_loads_host):
        f.restype = None
    return L


def host_loads(L, flat, op, derivatives=True):
    """rh_rotor_loads_host of a FlatRotor at op [n, 5]: loads [n,8], dloads [n,2,3], sec, status."""
    rec = flat.record()
    op = np.ascontiguousarray(op, dtype=float)
    n = len(op)
    loads, dl = np.zeros([n, 8]), np.zeros([n, 2, 3])
    sec = np.zeros([n, flat.nsector, flat.nr, 3])
    status = np.zeros(n, dtype=np.int32)
    L.rh_rotor_loads_host(ctypes.addressof(rec), n, op.ctypes.data, loads.ctypes.data,
                          dl.ctypes.data if derivatives else None, sec.ctypes.data, status.ctypes.data)
    return loads, dl, sec, status


def volturn_ccblade():
    """The CCBlade of VolturnUS-S_aero's rotor (the restatement class) and the rotor itself."""
    import raft
    from conftest import load_design
    m = raft.Model(load_design("VolturnUS-S_aero"))
    rot = m.fowtList[0].rnaList[0]
    return rot.ccblade, rot, m


def resampled(cc, nr, nsector, shear=None):
    """A raft.ccblade.CCBlade with nr stations taken from cc's blade (stations, chord, twist, curvature
    and airfoils at the nearest of cc's stations when resampling up, every few of them when down)
    and nsector sectors; nsector = 1 takes an axisymmetric inflow (no tilt, yaw or shear)."""
    from raft.ccblade import CCBlade
    n0 = len(cc.r)
    r = cc.Rhub + (cc.Rtip - cc.Rhub) * (np.arange(nr) + 0.5) / nr
    src = np.clip(np.round(np.interp(r, cc.r, np.arange(n0))).astype(int), 0, n0 - 1)
    axis = nsector == 1
    new = CCBlade(r, np.interp(r, cc.r, cc.chord), np.degrees(np.interp(r, cc.r, cc.theta)), [cc.af[i] for i in src],
                  cc.Rhub, cc.Rtip, cc.B, cc.rho, cc.mu, np.degrees(cc.precone), 0.0 if axis else np.degrees(cc.tilt),
                  0.0, 0.0 if axis else (cc.shearExp if shear is None else shear), cc.hubHt, nsector,
                  np.interp(r, cc.r, cc.precurve), cc.precurveTip, np.interp(r, cc.r, cc.presweep), cc.presweepTip,
                  derivatives=True, **cc.bemoptions)
    assert new.nSector == nsector
    return new


def python_reference(cc, points, tilt, yaw, derivs_at=()):
    """raft/ccblade.py at the points (Uinf, rpm, deg): loads [n,8], phi / Np / Tp [n,nsector,nr], and
    for the indices in derivs_at the derivatives d [6] = d(T, Q)/d(Uinf, Omega, pitch) with their bar:
    ten times the larger change of an entry when _solve_phi is shifted by +-4e-12, at least 1e-8 of
    the entry.  cc is left as it was."""
    keep = cc.tilt, cc.yaw, cc.derivatives
    cc.tilt, cc.yaw = tilt, yaw
    n, ns, nr = len(points), cc.nSector, len(cc.r)
    loads = np.zeros([n, 8])
    sec = np.zeros([n, ns, nr, 3])
    dref, dbar = {}, {}
    try:
        for p, (U, Om, pit) in enumerate(points):
            cc.derivatives = False
            seen, real_loads = [], cc.distributedAeroLoads

            def recorded(*a):                 # the sections evaluate() itself solved, sector after sector
                out = real_loads(*a)
                seen.append(out[0])
                return out
            cc.distributedAeroLoads = recorded
            try:
                L, _ = cc.evaluate(U, Om, pit)
            finally:
                del cc.distributedAeroLoads
            loads[p] = [L[k][0] for k in KEYS]
            for j in range(ns):
                sec[p, j] = np.stack([seen[j]["phi"], seen[j]["Np"], seen[j]["Tp"]], axis=1)
            if p in derivs_at:
                cc.derivatives = True

                def d6(shift):
                    real = type(cc)._solve_phi
                    cc._solve_phi = lambda rotating, args: real(cc, rotating, args) + shift
                    try:
                        _, D = cc.evaluate(U, Om, pit)
                    finally:
                        del cc._solve_phi
                    return np.array([D[a][b][0, 0] for a in ("dT", "dQ") for b in ("dUinf", "dOmega", "dpitch")])
                d0 = d6(0.0)
                change = np.maximum(np.abs(d6(4e-12) - d0), np.abs(d6(-4e-12) - d0))
                dref[p] = d0
                dbar[p] = np.maximum(10 * change, 1e-8 * np.abs(d0))
    finally:
        cc.tilt, cc.yaw, cc.derivatives = keep
    return dict(loads=loads, sec=sec, dref=dref, dbar=dbar)


def check_parity(ref, loads, sec, dloads, status, what):
    """The bars of the rotor parity checks on one rotor's points: phi to PHI_TOL per (sector, section)
    with Np, Tp to LOAD_TOL of the blade's largest, forces to LOAD_TOL |T| and moments to LOAD_TOL
    |Q|, and the self-calibrated derivative bars (which must stay below 1e-5 of the entry)."""
    for p in range(len(ref["loads"])):
        tag = f"{what} point {p}"
        assert status[p] == 0, (tag, status[p])
        dphi = np.abs(sec[p, :, :, 0] - ref["sec"][p, :, :, 0])
        j, i = np.unravel_index(np.argmax(dphi), dphi.shape)
        assert dphi.max() <= PHI_TOL, (tag, "phi", "sector", j, "section", i, dphi.max())
        for c, name in ((1, "Np"), (2, "Tp")):
            scale = np.abs(ref["sec"][p, :, :, c]).max()
            err = np.abs(sec[p, :, :, c] - ref["sec"][p, :, :, c])
            j, i = np.unravel_index(np.argmax(err), err.shape)
            assert err.max() <= LOAD_TOL * scale, (tag, name, "sector", j, "section", i, err.max(), scale)
        R = dict(zip(KEYS, ref["loads"][p]))
        G = dict(zip(KEYS, loads[p]))
        assert np.all(np.isfinite(ref["loads"][p])), tag
        for k in ("T", "Y", "Z"):
            assert abs(G[k] - R[k]) <= LOAD_TOL * abs(R["T"]), (tag, k, G[k], R[k])
        for k in ("Q", "My", "Mz", "Mb"):
            assert abs(G[k] - R[k]) <= LOAD_TOL * abs(R["Q"]), (tag, k, G[k], R[k])
        assert abs(G["P"] - R["P"]) <= LOAD_TOL * abs(R["P"]), (tag, "P", G["P"], R["P"])   # P = Q Omega pi / 30
        if p in ref["dref"]:
            d0, bar = ref["dref"][p], ref["dbar"][p]
            assert np.all(bar <= 1e-5 * np.abs(d0)), (tag, "a noisy derivative bar", bar / np.abs(d0))
            err = np.abs(np.asarray(dloads[p]).reshape(6) - d0)
            assert np.all(err <= bar), (tag, "derivatives", err / np.abs(d0), bar / np.abs(d0))

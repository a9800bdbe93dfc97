"""GPU: rotor blade-element momentum loads on the device (csrc/rh_rotor.hip through
raft/rotor_device.py, FOWT.rotorLoadsBatch and the rotor_device= keyword of the batched entry
points) against raft/ccblade.py and the host paths they replace.  Bars: phi to 1e-11 per (sector,
section), forces to 1e-9 |T|, moments to 1e-9 |Q|, the derivatives to their self-calibrated bars
(tests/helpers/rotor_cases.py).  Shapes are the smallest that exercise the lane grouping: nr = 1, 3,
20, 33, 64 (group widths 1, 4, 32, 64, 64), 1, 4 and 5 sectors, two rotors in one launch and 67
points.  The Python references are computed once per module and shared.

nr = 1: raft.ccblade.CCBlade cannot evaluate a blade of one station (define_curvature takes the
cone angle from the segments between stations), so that shape is the middle station of the
3-station rotor's record, compared with the host build of the same header (tools/rotor_host.cpp,
which tests/test_rotor_host.py ties to the Python) at the same bars.

Status 1 (a section without a sign change in any bracket): the search on the CPU found no such
section (tests/test_rotor_host.py::test_second_bracket_points), so that part of the status check
has no case and is left out; its phi = 0 path runs in the header's stand-alone program."""
import copy
import os
import sys

import numpy as np
import pytest

from conftest import load_design

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import rotor_cases as RC  # noqa: E402
from moor_array_cases import CASES  # noqa: E402

pytestmark = pytest.mark.gpu

# Measured on the device (MI355X), normwise relative difference between bem=device and the host path:
#   calcTurbineConstants: B_aero and f_aero 2.21e-11 (VolturnUS-S_aero), 1.31e-11 (OC3spar_aero); both designs
#                         have aeroServoMod 1, where A_aero is zero on both paths
#   analyzeCasesBatch Xi: 1.73e-13 (plain), 2.78e-13 (statics=True); analyzeArrayBatch(statics=True) Xi: 1.21e-12
# (B_aero and f_aero are dT/dUinf, a central difference that carries such noise itself).  The tests
# assert at ten times the measured value, and never above 1e-5.
AERO_MEASURED = {"VolturnUS-S_aero": 2.21e-11, "OC3spar_aero": 1.31e-11}
XI_MEASURED = 2.78e-13
XI_ARRAY_MEASURED = 1.21e-12
SHAPES = [(3, 4), (20, 4), (33, 5), (64, 4), (20, 1), (64, 1)]
TILT, YAW = 0.1, 0.05


def bar(measured):
    return min(10 * measured, 1e-5)


def nrm(a, b):
    b = np.asarray(b)
    return float(np.linalg.norm(np.asarray(a) - b) / max(np.linalg.norm(b), 1e-300))


@pytest.fixture(scope="module")
def base():
    return RC.volturn_ccblade()


@pytest.fixture(scope="module")
def rotors(base):
    """shape -> (CCBlade, points, reference, tilt, yaw); the 20 x 4 rotor is the design's own blade at
    the ten points and the five schedule points (with derivatives), the others take three points."""
    cc, rot, _ = base
    sched = [(U, float(np.interp(U, rot.Uhub, rot.Omega_rpm)), float(np.interp(U, rot.Uhub, rot.pitch_deg)))
             for U in RC.SCHEDULE_U]
    out = {}
    for nr, ns in SHAPES:
        tilt, yaw = (0.0, 0.0) if ns == 1 else (TILT, YAW)
        if (nr, ns) == (20, 4):
            pts = RC.POINTS + sched + RC.SECOND_BRACKET_POINTS
            ref = RC.python_reference(cc, pts, tilt, yaw, derivs_at=range(len(RC.POINTS), len(RC.POINTS) + len(sched)))
            out[nr, ns] = (cc, pts, ref, tilt, yaw)
        else:
            c2 = RC.resampled(cc, nr, ns)
            pts = [RC.POINTS[0], RC.POINTS[3], RC.POINTS[5]]
            out[nr, ns] = (c2, pts, RC.python_reference(c2, pts, tilt, yaw), tilt, yaw)
    return out


def device_eval(dr, idx, pts, tilt, yaw, derivatives=True):
    U, Om, pit = (np.array(v, dtype=float) for v in zip(*pts))
    loads, derivs, status, sec = dr.evaluate(idx, U, Om, pit, tilt, yaw, derivatives=derivatives, sections=True)
    L8 = np.stack([loads[k] for k in RC.KEYS], axis=1)
    D = (np.stack([np.diag(derivs[a][b]) for a in ("dT", "dQ") for b in ("dUinf", "dOmega", "dpitch")], axis=1)
         if derivatives else None)
    return L8, D, sec, status


# ------------------------------------------------------------------------------ parity, shape by shape
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"nr{s[0]}_ns{s[1]}")
def test_parity_against_python(rotors, shape):
    from raft.rotor_device import DeviceRotor
    cc, pts, ref, tilt, yaw = rotors[shape]
    dr = DeviceRotor([cc], 0)
    L8, D, sec, status = device_eval(dr, None, pts, tilt, yaw)
    assert sec.shape[1:] == (shape[1], shape[0], 3)
    RC.check_parity(ref, L8, sec, D, status, f"device nr={shape[0]} nSector={shape[1]}")
    if shape[1] == 1:
        assert np.all(L8[:, [1, 2, 4, 5]] == 0.0)               # Y, Z, My, Mz of an axisymmetric inflow


def test_one_station_against_the_host_header(rotors):
    """nr = 1 (group width 1): see the module's docstring."""
    from raft.rotor_device import DeviceRotor, FlatRotor, flatten_rotor
    cc, pts, _, tilt, yaw = rotors[3, 4]
    f3 = flatten_rotor(cc)
    one = FlatRotor(dict(f3.scalars, nr=1), f3.section[:, 1:2], f3.nknot[:, 1:2], f3.knots[:, 1:2], f3.coef[:, 1:2])
    op = np.array([[U, Om, pit, tilt, yaw] for U, Om, pit in pts], dtype=float)
    hl, hd, hsec, hst = RC.host_loads(RC.host_lib(), one, op)
    ref = dict(loads=hl, sec=hsec, dref={}, dbar={})
    L8, D, sec, status = device_eval(DeviceRotor([one], 0), None, pts, tilt, yaw)
    RC.check_parity(ref, L8, sec, D, status, "device nr=1")
    # the derivatives are central differences with steps of 1e-7 and 1e-6: a difference of one unit in the
    # last place (1e-16) of the residual or a load becomes 1e-9 of the entry per term, a few terms per entry
    assert np.all(np.abs(D.reshape(-1, 2, 3) - hd) <= 1e-7 * np.abs(hd))


def test_two_rotors_in_one_launch(rotors):
    """nr = 3 / 4 sectors and nr = 33 / 5 sectors side by side: the small rotor's groups carry padding
    sections and a padding sector; a rot_idx out of range gives status 3 for that row only."""
    from raft.rotor_device import DeviceRotor
    (ca, pa, ra, tilt, yaw), (cb, pb, rb, _, _) = rotors[3, 4], rotors[33, 5]
    dr = DeviceRotor([ca, cb], 0)
    idx = [0, 1, 0, 1, 0, 1, 7, -1]
    pts = [pa[0], pb[0], pa[1], pb[1], pa[2], pb[2], pa[0], pb[0]]
    L8, D, sec, status = device_eval(dr, idx, pts, tilt, yaw)
    assert list(status) == [0, 0, 0, 0, 0, 0, 3, 3]
    assert not np.any(L8[6:]) and not np.any(D[6:]) and not np.any(sec[6:])
    RC.check_parity(ra, L8[0:6:2], sec[0:6:2, :4, :3], D[0:6:2], status[0:6:2], "device, rotor 0 of two")
    RC.check_parity(rb, L8[1:6:2], sec[1:6:2], D[1:6:2], status[1:6:2], "device, rotor 1 of two")
    assert not np.any(sec[0:6:2, 4:]) and not np.any(sec[0:6:2, :, 3:])     # entries the small rotor lacks
    # ... and the rows beside a bad index are what they are without it
    L8b, Db, secb, _ = device_eval(dr, idx[:6], pts[:6], tilt, yaw)
    assert np.array_equal(L8[:6], L8b) and np.array_equal(D[:6], Db) and np.array_equal(sec[:6], secb)


def test_rows_are_independent(rotors):
    """Row 0 of a 67-point launch equals the 1-point launch bit for bit, a 3-point launch equals rows
    0..2, and dloads = NULL gives the same loads bits."""
    from raft.rotor_device import DeviceRotor
    cc, pts, _, tilt, yaw = rotors[20, 4]
    dr = DeviceRotor([cc], 0)
    many = [pts[k % len(pts)] for k in range(67)]
    L67, D67, s67, st67 = device_eval(dr, None, many, tilt, yaw)
    L1, D1, s1, _ = device_eval(dr, None, many[:1], tilt, yaw)
    L3, D3, s3, _ = device_eval(dr, None, many[:3], tilt, yaw)
    assert np.array_equal(L67[:1], L1) and np.array_equal(D67[:1], D1) and np.array_equal(s67[:1], s1)
    assert np.array_equal(L67[:3], L3) and np.array_equal(D67[:3], D3) and np.array_equal(s67[:3], s3)
    Ln, _, sn, stn = device_eval(dr, None, many, tilt, yaw, derivatives=False)
    assert np.array_equal(L67, Ln) and np.array_equal(s67, sn) and np.array_equal(st67, stn)
    assert np.array_equal(L67[len(pts):2 * len(pts)], L67[:len(pts)])      # the same point anywhere in the launch


# ------------------------------------------------------------------------------ the host paths it replaces
WIND = [dict(CASES["wind"]), dict(CASES["wind_wave_current"]),
        dict(CASES["wind_wave_current"], wind_speed=14, wind_heading=-20, turbulence=0.1),
        dict(CASES["wind"], wind_speed=22, wind_heading=5)]
PARKED = dict(CASES["wind_wave_current"], wind_speed=30, turbine_status="parked")


def count_launches(monkeypatch):
    """Wraps DeviceRotor.launch (rh_rotor_loads) with a counter; returns the list it appends to."""
    from raft.rotor_device import DeviceRotor
    real, calls = DeviceRotor.launch, []

    def counted(self, *a, **kw):
        calls.append(1)
        return real(self, *a, **kw)
    monkeypatch.setattr(DeviceRotor, "launch", counted)
    return calls


def fresh(design):
    """A newly built model for each side of a comparison: the host path keeps the rotor's yaw from
    one case to the next (Rotor.setPosition takes the hub's lever arm with the yaw the last case
    left), so two runs agree only from the same history."""
    import raft
    return raft.Model(load_design(design))


@pytest.mark.parametrize("design", ["VolturnUS-S_aero", "OC3spar_aero"])
def test_turbine_constants_with_device_loads(design):
    """FOWT.calcTurbineConstants(case, bem=device) against the host path: f_aero0 to 1e-9 of |T| times
    the lever arm, A_aero, B_aero and f_aero normwise at ten times the measured difference."""
    import raft
    m = raft.Model(load_design(design))
    fowt = m.fowtList[0]
    cases = [dict(c) for c in WIND[:3]]
    bems = fowt.rotorLoadsBatch(cases, m.device)
    worst = {}
    for case, bem in zip(cases, bems):
        fowt.calcTurbineConstants(dict(case), ptfm_pitch=0)
        host = {k: np.array(getattr(fowt, k)) for k in ("f_aero0", "A_aero", "B_aero", "f_aero", "B_gyro")}
        T = abs(fowt.rnaList[0].aero_thrust)
        fowt.calcTurbineConstants(dict(case), ptfm_pitch=0, bem=bem)
        lever = max(1.0, float(np.linalg.norm(fowt.rnaList[0].r_hub_rel)))
        assert np.all(np.abs(fowt.f_aero0[:3] - host["f_aero0"][:3]) <= 1e-9 * T)
        assert np.all(np.abs(fowt.f_aero0[3:] - host["f_aero0"][3:]) <= 1e-9 * T * lever)
        assert np.array_equal(fowt.B_gyro, host["B_gyro"])
        for k in ("A_aero", "B_aero", "f_aero"):
            if np.any(host[k]):
                worst[k] = max(worst.get(k, 0.0), nrm(getattr(fowt, k), host[k]))
            else:
                assert not np.any(getattr(fowt, k))
    print(f"{design}: normwise difference of bem=device from the host path: "
          + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert "B_aero" in worst and "f_aero" in worst
    assert max(worst.values()) <= bar(AERO_MEASURED[design]), worst


def test_statics_batch_with_device_rotor():
    """solveStaticsBatch(rotor_device=True) against False: offsets within 1e-6 m and 1e-8 rad (a 1e-9
    load error on 1.4e6 N over 7e4 N/m is 2e-8 m; the margin is 50 x), equal iters, status 0."""
    cases = [dict(CASES["wind"]), dict(CASES["wind_wave_current"]), dict(WIND[2]), dict(CASES["current"])]
    a = fresh("VolturnUS-S_aero").solveStaticsBatch(cases, rotor_device=False)
    b = fresh("VolturnUS-S_aero").solveStaticsBatch(cases, rotor_device=True)
    assert not np.any(a["status"]) and not np.any(b["status"])
    assert np.array_equal(a["iters"], b["iters"])
    assert np.all(np.abs(a["X"][:, :3] - b["X"][:, :3]) <= 1e-6) and np.all(np.abs(a["X"][:, 3:] - b["X"][:, 3:]) <= 1e-8)
    assert np.array_equal(a["X"][3], b["X"][3])                # no wind: no rotor load enters
    assert np.abs(a["X"][0, 0]) > 5.0                          # ... and the thrust moves the others


def test_statics_array_batch_with_device_rotor():
    """The same check for solveStaticsArrayBatch on VolturnUS-S_farm_aero, one case with a per-FOWT
    wind-speed list."""
    cases = [dict(CASES["wind"]), dict(CASES["wind_wave_current"], wind_speed=[10.0, 6.0])]
    a = fresh("VolturnUS-S_farm_aero").solveStaticsArrayBatch(cases, rotor_device=False)
    b = fresh("VolturnUS-S_farm_aero").solveStaticsArrayBatch(cases, rotor_device=True)
    assert not np.any(a["status"]) and not np.any(b["status"])
    assert np.array_equal(a["iters"], b["iters"])
    Xa, Xb = a["X"].reshape(2, -1, 6), b["X"].reshape(2, -1, 6)
    assert np.all(np.abs(Xa[:, :, :3] - Xb[:, :, :3]) <= 1e-6) and np.all(np.abs(Xa[:, :, 3:] - Xb[:, :, 3:]) <= 1e-8)
    assert np.all(np.abs(a["Xi0"].reshape(2, -1, 6)[:, :, 0]) > 1.0)       # the thrust moves both FOWTs


@pytest.mark.parametrize("statics", [False, True], ids=["plain", "statics"])
def test_analyze_cases_batch_with_device_rotor(statics, monkeypatch):
    """analyzeCasesBatch(rotor_device=True) against False: three wind cases and a parked one; identical
    drag iteration counts, Xi normwise at ten times the measured difference, the parked case's rows
    bit-equal (no rotor load enters them).  The rotor loads of the whole call come from exactly one
    launch, also with statics=True, where the statics and the per-pose designs share them."""
    cases = [copy.deepcopy(c) for c in (WIND[1], WIND[2], dict(WIND[3], wave_period=9, wave_height=3, wave_spectrum="JONSWAP",
                                                                wave_heading=20), PARKED)]
    a = fresh("VolturnUS-S_aero").analyzeCasesBatch(cases, statics=statics, rotor_device=False)
    launches = count_launches(monkeypatch)
    b = fresh("VolturnUS-S_aero").analyzeCasesBatch(cases, statics=statics, rotor_device=True)
    assert len(launches) == 1, len(launches)
    assert np.array_equal(a["iters"], b["iters"]) and np.array_equal(a["status"], b["status"])
    worst = max(nrm(b["Xi"][i], a["Xi"][i]) for i in range(3))
    print(f"analyzeCasesBatch(statics={statics}): Xi normwise difference {worst:.2e}")
    assert worst <= bar(XI_MEASURED), worst
    assert np.array_equal(a["Xi"][3], b["Xi"][3])
    for k in ("std", "psd"):
        assert np.array_equal(a[k][3], b[k][3])
    if statics:
        assert np.array_equal(a["statics_iters"], b["statics_iters"])
        assert not np.any(a["statics_status"]) and not np.any(b["statics_status"])
        assert np.array_equal(a["mean_offsets"][3], b["mean_offsets"][3])
        assert np.all(np.abs(a["mean_offsets"][:, :3] - b["mean_offsets"][:, :3]) <= 1e-6)


def test_failed_rotor_solve_raises(base, monkeypatch):
    """A non-zero status names the case and the status in a RuntimeError."""
    from raft.rotor_device import DeviceRotor
    _, _, m = base
    fowt = m.fowtList[0]
    real = DeviceRotor.launch

    def bad_index(self, rot_idx, op, **kw):
        return real(self, np.asarray(rot_idx) + np.array([0, 5], dtype=np.int32), op, **kw)
    monkeypatch.setattr(DeviceRotor, "launch", bad_index)
    with pytest.raises(RuntimeError, match="case 1, rotor 0: status 3"):
        fowt.rotorLoadsBatch([dict(CASES["wind"]), dict(CASES["wind"])], m.device)


def test_invalid_records_are_refused_before_the_launch(rotors):
    """Counts outside the limits, nr < 1 and knots that decrease are RH_EINVAL (ValueError) with a
    message, checked on the host before any launch."""
    from raft.rotor_device import DeviceRotor, FlatRotor, flatten_rotor
    cc, pts, _, tilt, yaw = rotors[3, 4]
    f = flatten_rotor(cc)

    def launch(**changes):
        knots = f.knots.copy()
        if changes.pop("bad_knots", False):
            knots[1, 2, 5] = knots[1, 2, 4] - 1.0
        bad = FlatRotor(dict(f.scalars, **changes), f.section, f.nknot, knots, f.coef)
        return device_eval(DeviceRotor([bad], 0), None, pts[:1], tilt, yaw)
    for changes, text in ((dict(nr=0), "nr=0"), (dict(nr=65), "nr=65"), (dict(nsector=17), "nsector=17"),
                          (dict(nsector=0), "nsector=0"), (dict(knot_stride=129), "knot_stride=129"),
                          (dict(kx=4), "kx=4"), (dict(bad_knots=True), "alpha knots decrease")):
        with pytest.raises(ValueError, match=text):
            launch(**changes)
    assert launch()[3][0] == 0


def test_analyze_array_batch_with_device_rotor(monkeypatch):
    """analyzeArrayBatch(statics=True, rotor_device=True) against False on VolturnUS-S_farm_aero, one case
    with a per-FOWT wind-speed list: equal statics and drag iteration counts, offsets within 1e-6 m and
    1e-8 rad, Xi normwise at ten times the measured difference; exactly one rotor launch per FOWT."""
    waves = dict(wave_spectrum="JONSWAP", wave_period=10, wave_height=4, wave_heading=-30)
    cases = [dict(CASES["wind"], **waves), dict(CASES["wind_wave_current"], wind_speed=[10.0, 6.0])]
    a = fresh("VolturnUS-S_farm_aero").analyzeArrayBatch(cases, statics=True, rotor_device=False)
    launches = count_launches(monkeypatch)
    farm = fresh("VolturnUS-S_farm_aero")
    b = farm.analyzeArrayBatch(cases, statics=True, rotor_device=True)
    assert len(launches) == farm.nFOWT == 2, len(launches)
    assert np.array_equal(a["iters"], b["iters"]) and np.array_equal(a["status"], b["status"])
    assert np.array_equal(a["statics_iters"], b["statics_iters"])
    assert not np.any(a["statics_status"]) and not np.any(b["statics_status"])
    Xa, Xb = a["mean_offsets"].reshape(2, -1, 6), b["mean_offsets"].reshape(2, -1, 6)
    assert np.all(np.abs(Xa[:, :, :3] - Xb[:, :, :3]) <= 1e-6) and np.all(np.abs(Xa[:, :, 3:] - Xb[:, :, 3:]) <= 1e-8)
    worst = max(nrm(b["Xi"][i], a["Xi"][i]) for i in range(2))
    print(f"analyzeArrayBatch(statics=True): Xi normwise difference {worst:.2e}")
    assert worst <= bar(XI_ARRAY_MEASURED), worst

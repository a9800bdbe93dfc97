"""Shared inputs of tests/test_moor_array_host.py and tests/test_gpu_moor_array.py: the farm load
cases, the four synthetic systems that reach each new branch of csrc/rh_moor_array.h, seeded
poses, and the Python reference of one evaluation (raft/mooring.py)."""
import copy

import numpy as np

from conftest import load_design

CASES = {   # the reference's tests/test_model.py:64-69 (as tests/test_mooring.py holds them)
    "wave": {"wind_speed": 0, "wind_heading": 0, "turbulence": 0, "turbine_status": "operating", "yaw_misalign": 0,
             "wave_spectrum": "JONSWAP", "wave_period": 10, "wave_height": 4, "wave_heading": -30,
             "current_speed": 0, "current_heading": 0},
    "current": {"wind_speed": 0, "wind_heading": 0, "turbulence": 0, "turbine_status": "operating", "yaw_misalign": 0,
                "wave_spectrum": "JONSWAP", "wave_period": 0, "wave_height": 0, "wave_heading": 0,
                "current_speed": 0.6, "current_heading": 15},
    "wind": {"wind_speed": 8, "wind_heading": 30, "turbulence": 0, "turbine_status": "operating", "yaw_misalign": 0,
             "wave_spectrum": "JONSWAP", "wave_period": 0, "wave_height": 0, "wave_heading": 0,
             "current_speed": 0, "current_heading": 0},
    "wind_wave_current": {"wind_speed": 8, "wind_heading": 30, "turbulence": 0, "turbine_status": "operating",
                          "yaw_misalign": 0, "wave_spectrum": "JONSWAP", "wave_period": 10, "wave_height": 4,
                          "wave_heading": -30, "current_speed": 0.6, "current_heading": 15},
}
KEYS = ["wave", "current", "wind", "wind_wave_current"]
TOL = 1e-9          # device / host-compiled C++ against the Python, of each array's largest entry
TOL_J = 1e-8        # the central-difference tension Jacobian


def farm_design(key="wave", own=False):
    """VolturnUS-S_farm (the _aero design for the wind cases); own=True gives FOWT 0 mooringID = 1, so
    that an own system and the array system are both present."""
    d = copy.deepcopy(load_design("VolturnUS-S_farm_aero" if key.startswith("wind") else "VolturnUS-S_farm"))
    if own:   # (the farm design's own mooring section is empty: the single VolturnUS-S's three lines in 200 m)
        d["mooring"] = copy.deepcopy(load_design("VolturnUS-S_test")["mooring"])
        d["array"]["data"][0][d["array"]["keys"].index("mooringID")] = 1
    return d


def farm_model(key="wave", own=False):
    import raft
    return raft.Model(farm_design(key, own))


def _base(depth=200.0):
    from raft.mooring import MooringSystem
    ms = MooringSystem(depth=depth)
    ms.add_line_type("chain", 0.2, 500.0, 1.0e9)
    ms.add_line_type("rope", 0.12, 40.0, 1.0e8)
    return ms


def _fair(ms, body, r):
    from raft.mooring import Point
    p = ms.add_point(Point.FIXED, np.asarray(body.r6[:3]) + np.asarray(r, dtype=float))
    body.attach(p, np.asarray(r, dtype=float))
    return p


def synthetic_systems():
    """name -> (MooringSystem, reference poses [nb, 6]); the smallest systems that reach each branch."""
    from raft.mooring import Point
    out = {}
    # one body in 600 m, a clump free point joining anchor - free - fairlead, plus one plain anchor line
    ms = _base(600.0)
    b = ms.add_body(np.zeros(6))
    a1, a2 = ms.add_point(Point.FIXED, [800.0, 0.0, -600.0]), ms.add_point(Point.FIXED, [-800.0, 0.0, -600.0])
    fr = ms.add_point(Point.FREE, [400.0, 0.0, -300.0], m=20000.0, v=1.0)
    f1, f2 = _fair(ms, b, [50.0, 0.0, -15.0]), _fair(ms, b, [-50.0, 0.0, -15.0])
    ms.add_line(520.0, "chain", a1, fr)
    ms.add_line(470.0, "chain", fr, f1)
    ms.add_line(1000.0, "chain", a2, f2)
    out["clump"] = (ms, np.zeros([1, 6]))
    # two bodies joined by one body-body line, one anchor line each, no free point
    ms = _base()
    X = np.array([[0.0, 0, 0, 0, 0, 0], [600.0, 0, 0, 0, 0, 0]])
    b1, b2 = ms.add_body(X[0]), ms.add_body(X[1])
    a1, a2 = ms.add_point(Point.FIXED, [-800.0, 0.0, -200.0]), ms.add_point(Point.FIXED, [1400.0, 0.0, -200.0])
    ms.add_line(850.0, "chain", a1, _fair(ms, b1, [-50.0, 0.0, -15.0]))
    ms.add_line(850.0, "chain", _fair(ms, b2, [50.0, 0.0, -15.0]), a2)          # attached end is A here
    ms.add_line(520.0, "rope", _fair(ms, b1, [50.0, 0.0, -15.0]), _fair(ms, b2, [-50.0, 0.0, -15.0]))
    out["two_bodies"] = (ms, X)
    # a line between two points of one body (and two anchor lines that hold the body)
    ms = _base()
    b = ms.add_body(np.zeros(6))
    a1, a2 = ms.add_point(Point.FIXED, [800.0, 0.0, -200.0]), ms.add_point(Point.FIXED, [-800.0, 0.0, -200.0])
    f1, f2 = _fair(ms, b, [50.0, 0.0, -15.0]), _fair(ms, b, [-50.0, 0.0, -15.0])
    ms.add_line(850.0, "chain", a1, f1)
    ms.add_line(850.0, "chain", a2, f2)
    ms.add_line(110.0, "rope", _fair(ms, b, [40.0, 30.0, -10.0]), _fair(ms, b, [-40.0, 30.0, -18.0]))
    out["same_body"] = (ms, np.zeros([1, 6]))
    # 8 free points in a chain (the limit) in 600 m: anchor - 8 clumps - fairlead, and a plain anchor line opposite
    ms = _base(600.0)
    b = ms.add_body(np.zeros(6))
    prev = ms.add_point(Point.FIXED, [800.0, 0.0, -600.0])
    for i in range(8):
        p = ms.add_point(Point.FREE, [800.0 - 750.0 / 9 * (i + 1), 0.0, -600.0 + 65.0 * (i + 1)], m=1000.0)
        ms.add_line(112.0, "rope", prev, p)
        prev = p
    ms.add_line(112.0, "rope", prev, _fair(ms, b, [50.0, 0.0, -15.0]))
    ms.add_line(1000.0, "chain", ms.add_point(Point.FIXED, [-800.0, 0.0, -600.0]), _fair(ms, b, [-50.0, 0.0, -15.0]))
    out["chain8"] = (ms, np.zeros([1, 6]))
    for ms, _ in out.values():
        ms.initialize()
    return out


def seeded_poses(X_ref, n, seed):
    """n poses about X_ref [nb, 6]: +-20 m, +-0.1 rad, heave x 0.25."""
    rng = np.random.default_rng(seed)
    d = np.concatenate([rng.uniform(-20, 20, [n, len(X_ref), 3]), rng.uniform(-0.1, 0.1, [n, len(X_ref), 3])], axis=2)
    d[:, :, 2] *= 0.25
    return np.asarray(X_ref)[None] + d


def get_state(ms):
    return [(ln.HF, ln.VF) for ln in ms.lines], [p.r.copy() for p in ms.points], [b.r6.copy() for b in ms.bodies]


def set_state(ms, state):
    for ln, (hf, vf) in zip(ms.lines, state[0]):
        ln.HF, ln.VF = hf, vf
    for p, r in zip(ms.points, state[1]):
        p.r = r.copy()
    for b, r6 in zip(ms.bodies, state[2]):
        b.r6 = r6.copy()


def python_eval(ms, r6, state, jacobian=True):
    """raft/mooring.py at body poses r6 [nb, 6], started from `state` (get_state): F, K (analytic,
    condensed), T, J, the solved warm state and free points, and the _solve_lines passes of the
    pose's own equilibrium."""
    from raft.mooring import Point
    set_state(ms, state)
    count, real = [0], ms._solve_lines

    def counted():
        count[0] += 1
        real()
    ms._solve_lines = counted
    try:
        ms.set_body_positions(list(r6))
    finally:
        del ms._solve_lines
    out = dict(F=ms.coupled_forces(lines_only=True), K=ms.coupled_stiffness_analytic(), T=ms.tensions(), nev=count[0],
               warm=np.array([[ln.HF, ln.VF] for ln in ms.lines]),
               free=np.array([p.r for p in ms.points if p.type == Point.FREE]).reshape(-1, 3))
    if jacobian:
        out["J"] = ms.coupled_stiffness_fd(tensions=True)[1]
    return out


def rel(a, b):
    b = np.asarray(b)
    return float(np.abs(np.asarray(a) - b).max() / max(np.abs(b).max(), 1e-300)) if b.size else 0.0

"""Inputs and host references of the tests of current on the mooring lines (tests/test_moor_current_host.py
on the CPU, tests/test_gpu_moor_current.py on the device): the synthetic systems of tests/test_gpu_moor.py
rebuilt with line types that carry drag (without Cd / CdAx a current does nothing to a line), seeded
horizontal currents up to 1.5 m/s at any heading (the range in which the host solves every input, the
central-difference Jacobian included), single lines for each branch of Line.static_solve(current=...),
and the two single-FOWT designs with mooring currentMod = 1."""
import numpy as np

UMAX = 1.5          # m/s: the host solves every pose of the systems below up to here


def synthetic_drag(kind):
    """tests/test_gpu_moor.py's synthetic(kind) -- "one" (1 line), "four" (fills its group), "five" (group
    of 8: one line vessel-end-first, one anchor off the seabed, one taut rope) -- with chain (Cd 1.2,
    CdAx 0.2) and rope (Cd 1.6, CdAx 0.1)."""
    from raft.mooring import MooringSystem, Point
    ms = MooringSystem(depth=200.0)
    ms.add_line_type("chain", 0.15, 350.0, 1.5e9, 1.2, 0.2)
    ms.add_line_type("rope", 0.12, 30.0, 2.0e8, 1.6, 0.1)
    body = ms.add_body(np.zeros(6))

    def line(ang, L, ltype="chain", radius=820.0, za=-200.0, vessel_first=False, zf=-14.0):
        c, s = np.cos(np.radians(ang)), np.sin(np.radians(ang))
        anchor = ms.add_point(Point.FIXED, [radius * c, radius * s, za])
        fair = ms.add_point(Point.FIXED, [45.0 * c, 45.0 * s, zf])
        body.attach(fair, fair.r.copy())
        ms.add_line(L, ltype, *((fair, anchor) if vessel_first else (anchor, fair)))

    if kind == "one":
        line(20.0, 850.0)
    elif kind == "four":
        for a in (10.0, 100.0, 190.0, 280.0):
            line(a, 850.0)
    else:
        line(0.0, 850.0)
        line(72.0, 850.0, vessel_first=True)
        line(144.0, 840.0, za=-190.0)                                         # anchor off the seabed
        line(216.0, 0.995 * np.hypot(775.0, 186.0), ltype="rope")              # taut
        line(288.0, 870.0, zf=-20.0)
    ms.initialize()
    return ms


def single_line(ltype, anchor, fair, L, depth=200.0, vessel_first=False):
    """A one-line system: `anchor` fixed, `fair` attached to the body (at the origin).
    ltype = (d, mass per length, EA, Cd, CdAx)."""
    from raft.mooring import MooringSystem, Point
    ms = MooringSystem(depth=depth)
    ms.add_line_type("t", *ltype)
    body = ms.add_body(np.zeros(6))
    a = ms.add_point(Point.FIXED, list(anchor))
    b = ms.add_point(Point.FIXED, list(fair))
    body.attach(b, b.r.copy())
    ms.add_line(L, "t", *((b, a) if vessel_first else (a, b)))
    return ms


CHAIN = (0.185, 685.0, 3270e6, 1.6, 0.1)        # tests/test_mooring.py's suspended chain
HEAVY = (0.15, 40.0, 500e6, 1.2, 0.1)           # its heavy line of the ordering flip (net weight 215 N/m)
LIGHT = (0.3, 75.0, 500e6, 1.2, 0.1)            # wet weight 25 N/m: a rising current lifts it
# name -> (system arguments, current): every branch of Line.static_solve(current=...)
LINE_CASES = {
    "suspended": (dict(ltype=CHAIN, anchor=[0.0, 0.0, -150.0], fair=[300.0, 40.0, -14.0], L=360.0), [0.3, -0.9, 0.0]),
    "seabed": (dict(ltype=CHAIN, anchor=[800.0, 100.0, -200.0], fair=[45.0, 5.0, -14.0], L=850.0), [1.0, 0.5, 0.0]),
    "off_seabed": (dict(ltype=CHAIN, anchor=[800.0, 0.0, -190.0], fair=[45.0, 0.0, -14.0], L=840.0), [-0.7, 1.1, 0.0]),
    "taut": (dict(ltype=CHAIN, anchor=[775.0, 0.0, -200.0], fair=[0.0, 0.0, -14.0], L=0.995 * np.hypot(775.0, 186.0)),
             [0.0, 1.5, 0.0]),
    "vessel_first": (dict(ltype=CHAIN, anchor=[-600.0, 550.0, -200.0], fair=[-30.0, 30.0, -14.0], L=850.0,
                          vessel_first=True), [1.2, 0.4, 0.0]),
    "flip_3.5": (dict(ltype=HEAVY, anchor=[-220.0, 0.0, -200.0], fair=[0.0, 0.0, -20.0], L=300.0), [3.5, 0.0, 0.0]),
    "flip_4.0": (dict(ltype=HEAVY, anchor=[-220.0, 0.0, -200.0], fair=[0.0, 0.0, -20.0], L=300.0), [4.0, 0.0, 0.0]),
    "up": (dict(ltype=LIGHT, anchor=[0.0, 0.0, -180.0], fair=[150.0, 20.0, -60.0], L=200.0), [0.4, 0.1, 0.8]),
}


def poses(n, seed):
    """tests/test_gpu_moor.py's seeded poses."""
    rng = np.random.default_rng(seed)
    r6 = np.concatenate([rng.uniform(-20, 20, [n, 3]), rng.uniform(-0.1, 0.1, [n, 3])], axis=1)
    r6[:, 2] *= 0.25
    return r6


def currents(n, seed, zero_every=0):
    """Seeded horizontal currents [n, 3]: speed in (0, UMAX], any heading; every `zero_every`-th row zero."""
    rng = np.random.default_rng(1000 + seed)
    sp, hd = UMAX * (1.0 - rng.uniform(0.0, 1.0, n)), rng.uniform(0.0, 2 * np.pi, n)
    U = np.stack([sp * np.cos(hd), sp * np.sin(hd), np.zeros(n)], axis=1)
    if zero_every:
        U[::zero_every] = 0.0
    return U


def host_reference(ms, r6s, U):
    """F, K, T, J and the warm states before / after each pose on the host system with ms.current = U[ip].
    Odd poses start cold, even poses warm from the pose before.  The host must solve every input: an
    exception of a pose is collected and asserted on, none is skipped.  ms.current is cleared at the end."""
    body = ms.bodies[0]
    out = dict(F=[], K=[], T=[], J=[], warm_in=[], warm_out=[])
    failed = []
    for ip, r6 in enumerate(r6s):
        if ip % 2:
            for ln in ms.lines:
                ln.HF = ln.VF = 0.0
        out["warm_in"].append([[ln.HF, ln.VF] for ln in ms.lines])
        ms.current = np.array(U[ip], dtype=float)
        try:
            ms.set_body_positions([r6])
            row = (ms.body_forces(body), ms.coupled_stiffness_analytic(), ms.tensions(),
                   ms.coupled_stiffness_fd(tensions=True)[1])
        except (RuntimeError, ValueError, ZeroDivisionError, OverflowError) as e:
            failed.append((ip, repr(e)))
            continue
        for k, v in zip("FKTJ", row):
            out[k].append(v)
        out["warm_out"].append([[ln.HF, ln.VF] for ln in ms.lines])
    ms.current = np.zeros(3)
    assert not failed, failed
    return {k: np.array(v) for k, v in out.items()}


def current_design(name):
    """A design of tests/golden/designs with mooring currentMod = 1."""
    from conftest import load_design
    d = load_design(name)
    d["mooring"]["currentMod"] = 1
    return d


def seeded_case(base, seed):
    """`base` with a seeded current speed in (0, UMAX] and heading."""
    rng = np.random.default_rng(seed)
    return dict(base, current_speed=float(UMAX * (1.0 - rng.uniform(0.0, 1.0))), current_heading=float(rng.uniform(0, 360)))

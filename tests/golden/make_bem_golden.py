"""Generate the potential-flow coefficient-file fixtures (potFirstOrder = 1) by running the
READ-ONLY reference inside the build container, following make_golden.py's recipe
(prepare_fowt, C_MOOR, wind_speed = 0, iteration counts from display=2).

Run (from the repo root, in the build container):

    PYTHONDONTWRITEBYTECODE=1 OPENBLAS_NUM_THREADS=1 \
    PYTHONPATH=tests/golden/refshim:/root/reference python tests/golden/make_bem_golden.py

tests/golden/refshim/pyhams stands in for pyHAMS: its read_wamit1 / read_wamit3 are the project's
own reader (raft/bem_io.py), so what is pinned here is everything downstream of the reader.

Writes
  tests/golden/bem/synth.1, synth.3           synthetic WAMIT-format pair from closed-form functions:
                                              periods -1, 0 and 10 finite ones; headings 0, 90, 180, -90
  tests/golden/bem/synth_unsorted.1, .3       the same data with the .3 headings in the order 180, -90, 0, 90
  tests/golden/bem_a.npz .. bem_e.npz         reference inputs and outputs (see each function)
tests/golden/bem/Buoy.1, Buoy.3 are the reference's own data files
(raft/data/cylinder/Output/Wamit_format), copied as data.
"""
import contextlib
import io
import json
import os
import re
import sys

import numpy as np

import raft  # the reference, from PYTHONPATH
import raft.raft_fowt as rf

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import C_MOOR, K_ARRAY, REF, load_design, prepare_fowt, run_solve, seeded_cases  # noqa: E402

BEM = os.path.join(HERE, "bem")
GRID = dict(min_freq=0.02, max_freq=0.4)      # nw = 20
PERIODS = [80.0, 60.0, 45.0, 30.0, 20.0, 12.0, 8.0, 5.0, 3.5, 2.2]   # two longer than the grid's 50 s, one shorter than 2.5 s
SEED = 20241101


def synth_AB(w, rng_tab):
    """Symmetric 6x6 A(w), B(w) in the files' units (divided by rho)."""
    dA = np.array([8.0e3, 8.0e3, 3.0e2, 4.0e6, 4.0e6, 1.0e2])
    dB = np.array([3.0e2, 3.0e2, 5.0, 1.0e5, 1.0e5, 1.0])
    A = np.diag(dA * (1.0 + 0.3 / (1.0 + w * w)))
    B = np.diag(dB * w * w * np.exp(-1.5 * w))
    A[0, 4] = A[4, 0] = -6.0e4 * (1.0 + 0.2 * np.cos(w))
    A[1, 3] = A[3, 1] = 6.0e4 * (1.0 + 0.2 * np.cos(w))
    B[0, 4] = B[4, 0] = -2.0e3 * w * w * np.exp(-1.5 * w)
    B[1, 3] = B[3, 1] = 2.0e3 * w * w * np.exp(-1.5 * w)
    return A * (1.0 + 0.01 * rng_tab), B * (1.0 + 0.01 * rng_tab)


def synth_X(w, hdeg):
    """Excitation / (rho g) in the global frame for a wave from heading hdeg."""
    h = np.radians(hdeg)
    shape = 1.0 + 0.1 * np.cos(3 * h)
    ph = np.exp(1j * (0.3 + 0.5 * w))
    Fs = 1.0e2 * w * np.exp(-0.8 * w) * shape
    Fh = 3.0e1 * np.exp(-1.2 * w) * shape
    Mp = 4.0e3 * w * np.exp(-0.9 * w) * shape
    return np.array([Fs * np.cos(h) * ph, Fs * np.sin(h) * ph, Fh * np.conj(ph), -Mp * np.sin(h) * 1j * ph,
                     Mp * np.cos(h) * 1j * ph, 2.0 * np.sin(2 * h) * w * ph])


def write_synthetic():
    rng = np.random.default_rng(SEED)
    tab = rng.uniform(-1, 1, [6, 6])
    tab = 0.5 * (tab + tab.T)
    for name in ("synth", "synth_unsorted"):
        with open(os.path.join(BEM, name + ".1"), "w") as f:
            for T in [-1.0, 0.0] + PERIODS:
                w = 0.0 if T < 0 else (50.0 if T == 0 else 2 * np.pi / T)      # (the w = inf row: a large frequency)
                A, B = synth_AB(w, tab)
                for i in range(6):
                    for j in range(6):
                        if A[i, j] == 0 and B[i, j] == 0:
                            continue                                         # absent entries are zero
                        if T <= 0:
                            f.write(f" {T: .6E} {i + 1:5d} {j + 1:5d} {A[i, j]: .6E}\n")
                        else:
                            f.write(f" {T: .6E} {i + 1:5d} {j + 1:5d} {A[i, j]: .6E} {B[i, j]: .6E}\n")
    for name, heads in (("synth", [0.0, 90.0, 180.0, -90.0]), ("synth_unsorted", [180.0, -90.0, 0.0, 90.0])):
        with open(os.path.join(BEM, name + ".3"), "w") as f:
            for T in PERIODS:
                for hd in heads:
                    X = synth_X(2 * np.pi / T, hd)
                    for i in range(6):
                        f.write(f" {T: .6E} {hd: .6E} {i + 1:5d} {abs(X[i]): .6E} {np.degrees(np.angle(X[i])): .6E} "
                                f"{X[i].real: .6E} {X[i].imag: .6E}\n")
    print("wrote bem/synth*.1/.3", file=sys.stderr)


def bem_design(hydro, master):
    d = load_design(os.path.join(REF, "designs", "OC3spar.yaml"), **GRID)
    d["platform"].update(potFirstOrder=1, potModMaster=master, hydroPath=os.path.join(BEM, hydro))
    return d


def statics(fowt):
    out = {k: np.array(getattr(fowt, k), dtype=float) for k in
           ["M_struc", "B_struc", "C_struc", "C_hydro", "C_moor", "A_hydro_morison", "W_struc", "W_hydro"]}
    out["r6"] = fowt.r6.copy()
    out["w"] = fowt.w.copy()
    return out


def bem_arrays(fowt):
    return dict(A_BEM=fowt.A_BEM.copy(), B_BEM=fowt.B_BEM.copy(), X_BEM=fowt.X_BEM.copy(),
                BEM_headings=np.array(fowt.BEM_headings, dtype=float))


def golden_bem_solve(tag, hydro, master, cases):
    """Model.solveDynamics of OC3spar with the coefficient files `hydro`: the interpolated tables,
    and per case Xi, Z, iterations, F_BEM, F_hydro_iner, motion std / PSD."""
    model = raft.Model(bem_design(hydro, master))
    fowt = model.fowtList[0]
    if master == 3:
        fowt.calcBEM()                                  # as analyzeCases (raft/raft_model.py:258-263)
    out = {}
    res = {k: [] for k in ["Xi", "iters", "conv", "Z", "F_BEM", "F_iner", "B_drag", "std", "PSD"]}
    for c in cases:
        case = dict(c)
        prepare_fowt(fowt, case)
        if not out:
            out.update(statics(fowt))
            out.update(bem_arrays(fowt))
        Xi, iters, conv, dt = run_solve(model, case)
        m = {}
        fowt.saveTurbineOutputs(m, case)
        dofs = ["surge", "sway", "heave", "roll", "pitch", "yaw"]
        res["Xi"].append(Xi)
        res["iters"].append(iters)
        res["conv"].append(conv)
        res["Z"].append(fowt.Z.copy())
        res["F_BEM"].append(fowt.F_BEM.copy())
        res["F_iner"].append(fowt.F_hydro_iner.copy())
        res["B_drag"].append(fowt.B_hydro_drag.copy())
        res["std"].append(np.array([m[f"{d}_std"] for d in dofs]))
        res["PSD"].append(np.array([m[f"{d}_PSD"] for d in dofs]))
        print(f"  {tag}: heading {c['wave_heading']} iters={iters} conv={conv}", file=sys.stderr)
    for k, v in res.items():
        if k in ("Xi", "F_BEM", "F_iner") and len({np.shape(x) for x in v}) > 1:   # cases with 1 and 2 sea states
            for i, x in enumerate(v):
                out[f"out_{k}_{i}"] = np.array(x)
        else:
            out["out_" + k] = np.array(v)
    out["nIter"] = np.int64(model.nIter)
    out["XiStart"] = np.float64(model.XiStart)
    keys = ["wave_spectrum", "wave_period", "wave_height", "wave_heading", "wave_gamma"]
    out["cases_json"] = np.array(json.dumps([{k: np.atleast_1d(c[k]).tolist() for k in keys} for c in cases]))
    np.savez_compressed(os.path.join(HERE, f"{tag}.npz"), **out)
    print(f"wrote {tag}.npz", file=sys.stderr)


def sea(heading, period, height, gamma=0.0):
    n = len(heading) if isinstance(heading, list) else 0
    return dict(wind_speed=0, wind_heading=0, turbulence=0, turbine_status="operating", yaw_misalign=0,
                wave_spectrum=["JONSWAP"] * n if n else "JONSWAP", wave_period=period, wave_height=height,
                wave_heading=heading, wave_gamma=gamma)


def cases_b():
    rng = np.random.default_rng(SEED + 1)
    tp = [float(x) for x in rng.uniform(6.0, 16.0, 4)]
    hs = [float(x) for x in rng.uniform(1.0, 8.0, 4)]
    return [sea([30.0, 200.0], [tp[0], tp[1]], [hs[0], hs[1]], [0.0, 0.0]),     # two sea states
            sea(90.0, tp[2], hs[2]),                                            # exactly a file heading: the tie
            sea(300.0, tp[3], hs[3])]                                           # above the last heading: the wrap


def golden_fowt_level():
    """(d) One reference FOWT at x_ref = 30, y_ref = -20, heading_adjust = 25 with OC3spar's own
    potMod flags (potModMaster 0: the spar is a potMod member, so F_BEM applies and the tables are
    readHydro's, unsorted): calcHydroExcitation at headings 0, 25, 100 and 355."""
    d = bem_design("synth", 0)
    model = raft.Model(d)
    fowt = rf.FOWT(d, model.w, None, depth=model.depth, x_ref=30.0, y_ref=-20.0, heading_adjust=25.0)
    fowt.setPosition(np.array([fowt.x_ref, fowt.y_ref, 0, 0, 0, 0], dtype=float))
    fowt.calcStatics()
    fowt.calcHydroConstants()
    fowt.C_moor = C_MOOR.copy()
    out = statics(fowt)
    out.update(bem_arrays(fowt))
    heads = [0.0, 25.0, 100.0, 355.0]
    case = sea(heads, [10.0] * 4, [4.0] * 4, [0.0] * 4)
    cj = json.dumps([{k: case[k] for k in ["wave_spectrum", "wave_period", "wave_height", "wave_heading", "wave_gamma"]}])
    fowt.calcHydroExcitation(case, memberList=fowt.memberList)
    out.update(out_F_BEM=fowt.F_BEM.copy(), out_F_iner=fowt.F_hydro_iner.copy(), out_zeta=fowt.zeta.copy(),
               x_ref=np.float64(30.0), y_ref=np.float64(-20.0), heading_adjust=np.float64(25.0),
               cases_json=np.array(cj))
    np.savez_compressed(os.path.join(HERE, "bem_d.npz"), **out)
    print("wrote bem_d.npz", file=sys.stderr)


def golden_farm_bem():
    """(e) The two-FOWT farm (golden_farm's recipe: the farm design, K_ARRAY) on the nw = 20 grid,
    both FOWTs with potFirstOrder 1 + potModMaster 3 on the synthetic files: Xi of the system."""
    design = load_design(os.path.join(REF, "tests", "test_data", "VolturnUS-S_farm.yaml"), **GRID)
    for key in ("platform", "platforms"):
        ps = design.get(key)
        for p in (ps if isinstance(ps, list) else [ps] if ps else []):
            p.update(potFirstOrder=1, potModMaster=3, hydroPath=os.path.join(BEM, "synth"))
    model = raft.Model(design)
    model.ms.getCoupledStiffnessA = lambda *a, **kw: K_ARRAY.copy()
    for fowt in model.fowtList:
        fowt.calcBEM()
    case = seeded_cases(1, SEED + 2, headings=(40.0,))[0]
    out = {"K_array": K_ARRAY, "nIter": np.int64(model.nIter), "XiStart": np.float64(model.XiStart)}
    for i, fowt in enumerate(model.fowtList):
        prepare_fowt(fowt, dict(case))
        out.update({f"f{i}_{k}": v for k, v in statics(fowt).items()})
        out.update({f"f{i}_{k}": v for k, v in bem_arrays(fowt).items()})
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        Xi = model.solveDynamics(dict(case), display=2)
    its = [int(m) + 1 for m in re.findall(r"Iteration (\d+), converged", buf.getvalue())]
    assert len(its) == len(model.fowtList), its
    out.update(out_Xi=np.array(Xi), out_iters=np.array(its),
               out_F_BEM=np.array([f.F_BEM.copy() for f in model.fowtList]))
    keys = ["wave_spectrum", "wave_period", "wave_height", "wave_heading", "wave_gamma"]
    out["cases_json"] = np.array(json.dumps([{k: np.atleast_1d(case[k]).tolist() for k in keys}]))
    np.savez_compressed(os.path.join(HERE, "bem_e.npz"), **out)
    print(f"wrote bem_e.npz (iters {its})", file=sys.stderr)


def main():
    write_synthetic()
    golden_bem_solve("bem_a", "Buoy", 1, seeded_cases(3, SEED))
    golden_bem_solve("bem_b", "synth", 3, cases_b())
    golden_bem_solve("bem_c", "synth_unsorted", 3, [sea(135.0, 9.0, 5.0)])
    golden_fowt_level()
    golden_farm_bem()


if __name__ == "__main__":
    main()

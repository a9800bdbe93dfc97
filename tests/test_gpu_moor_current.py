"""GPU: current on the mooring lines in the batched mooring evaluation and mean-offset solve
(k_moor_eval_current / k_statics_solve_current of csrc/rh_moor_current.hip through DeviceMooring.eval /
solve_statics(current=...), Model.solveStaticsBatch(line_current=True) and analyzeCasesBatch(statics=True,
line_current=True)) against the host MooringSystem with .current set, Model.solveStatics and solveDynamics on
the mooring currentMod 1 designs, at the device parity convention of tests/test_gpu_moor.py (1e-9 of each
array's largest entry).  Shapes are the smallest that exercise the lane grouping: 1 line in a group of 1,
4 in 4, 5 in 8, 3 in 4 over 67 poses (a partial last wave), and two systems in one call.  Inputs and host
references: tests/helpers/moor_current_cases.py (every input is one the host solves, which is asserted);
references are computed once per module and shared."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import moor_current_cases as C  # noqa: E402
from test_moor_host import CASES, DESIGNS  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-9                       # tests/test_gpu_moor.py's: of each array's largest entry


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max()


# ------------------------------------------------------------------------------ evaluation
_CACHE = {}


def system_with_reference(name):
    """(system, poses, currents, host reference), built once.  "volturn": the 3-line system of
    VolturnUS-S_test (its line type carries drag) at 67 poses, every third current zero."""
    if name not in _CACHE:
        if name == "volturn":
            import raft
            ms = raft.Model(C.current_design(DESIGNS[0])).fowtList[0].ms
            r6s, U = C.poses(67, seed=7), C.currents(67, seed=7, zero_every=3)
        elif name == "flip":
            ms = C.single_line(**C.LINE_CASES["flip_3.5"][0])
            r6s = np.concatenate([np.zeros([2, 6]), C.poses(5, seed=4) * 0.25])
            U = np.array([[3.5, 0.0, 0.0], [4.0, 0.0, 0.0]] + [[3.5 + 0.1 * i, 0.2, 0.0] for i in range(5)])
        else:
            ms = C.synthetic_drag(name)
            r6s, U = C.poses(7, seed=len(name)), C.currents(7, seed=len(name))
        _CACHE[name] = (ms, r6s, U, C.host_reference(ms, r6s, U))
        assert len(_CACHE[name][3]["F"]) == len(r6s)       # the host solved every input
    return _CACHE[name]


def check_eval(got, ref, sl, nl, nl_max, rows=None):
    """Device tensors of DeviceMooring.eval (rows `rows` of them) against host rows sl."""
    g = {k: got[k].cpu().numpy() for k in ("F", "K", "T", "J", "status", "warm")}
    if rows is not None:
        g = {k: v[rows] for k, v in g.items()}
    assert not g["status"].any(), g["status"]
    cols = np.r_[0:nl, nl_max:nl_max + nl]
    errs = dict(F=rel(g["F"], ref["F"][sl]), K=rel(g["K"], ref["K"][sl]), T=rel(g["T"][:, cols], ref["T"][sl]),
                J=rel(g["J"][:, cols], ref["J"][sl]), warm=rel(g["warm"][:, :nl], ref["warm_out"][sl]))
    print("rh_moor_eval_current residuals", {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) < TOL, errs
    pad = np.setdiff1d(np.arange(2 * nl_max), cols)
    assert not g["T"][:, pad].any() and not g["J"][:, pad].any() and not g["warm"][:, nl:].any()


@pytest.mark.parametrize("kind", ["one", "four", "five"])
def test_moor_eval_current_synthetic(kind):
    """Groups of 1, 4 and 8: 7 poses with per-pose currents, odd poses cold and even poses warm."""
    from raft.mooring_device import DeviceMooring
    ms, r6s, U, ref = system_with_reference(kind)
    nl = len(ms.lines)
    dm = DeviceMooring([ms])
    got = dm.eval(r6s, warm=ref["warm_in"], jacobian=True, current=U)
    check_eval(got, ref, slice(None), nl, nl)
    calm = dm.eval(r6s, warm=ref["warm_in"], jacobian=True)
    assert rel(calm["F"].cpu().numpy(), ref["F"]) > 1e-6        # the current is felt
    # two systems' padding: one more column than the system has lines
    if kind == "one":
        ms4 = system_with_reference("four")[0]
        dm2 = DeviceMooring([ms, ms4])
        got2 = dm2.eval(r6s, sys_idx=np.zeros(len(r6s), dtype=np.int32), warm=np.pad(ref["warm_in"], ((0, 0), (0, 3), (0, 0))),
                        jacobian=True, current=U)
        check_eval(got2, ref, slice(None), 1, 4)


def test_moor_eval_current_partial_wave_and_neighbours():
    """67 poses of a 3-line system (groups of 4: 268 lanes, a partial last wave) against the host; rows with
    zero current are eval() without current bit for bit; row 0 equals the one-pose call bit for bit."""
    from raft.mooring_device import DeviceMooring
    ms, r6s, U, ref = system_with_reference("volturn")
    dm = DeviceMooring([ms])
    assert dm.nl_max == 3
    got = dm.eval(r6s, warm=ref["warm_in"], jacobian=True, current=U)
    check_eval(got, ref, slice(None), 3, 3)
    plain = dm.eval(r6s, warm=ref["warm_in"], jacobian=True)
    zero = ~U.any(axis=1)
    assert zero.sum() == 23 and not zero[1]
    for k in ("F", "K", "T", "J", "status", "warm"):
        a, b = got[k].cpu().numpy(), plain[k].cpu().numpy()
        assert a[zero].tobytes() == b[zero].tobytes(), k
        assert k in ("status",) or not np.array_equal(a[~zero], b[~zero]), k
    for row in (1, 66):
        one = dm.eval(r6s[row:row + 1], warm=ref["warm_in"][row:row + 1], jacobian=True, current=U[row:row + 1])
        for k in ("F", "K", "T", "J", "status", "warm"):
            assert one[k].cpu().numpy()[0].tobytes() == got[k].cpu().numpy()[row].tobytes(), (row, k)
    one = dm.eval(r6s[:1], warm=ref["warm_in"][:1], jacobian=True, current=U[:1])
    for k in ("F", "K", "T", "J", "status", "warm"):
        assert one[k].cpu().numpy()[0].tobytes() == got[k].cpu().numpy()[0].tobytes(), k


def test_moor_eval_current_two_systems():
    """nsys = 2 with mixed sys_idx: 3-line and 5-line poses interleaved in one call (groups of 8), each
    system with its own drag columns, each pose with its own current."""
    from raft.mooring_device import DeviceMooring
    ms3, r3, U3, ref3 = system_with_reference("volturn")
    ms5, r5, U5, ref5 = system_with_reference("five")
    n = len(r5)
    idx = np.array([0, 1] * n, dtype=np.int32)
    r6, U = np.empty([2 * n, 6]), np.empty([2 * n, 3])
    r6[0::2], r6[1::2] = r3[:n], r5
    U[0::2], U[1::2] = U3[:n], U5
    warm = np.zeros([2 * n, 5, 2])
    warm[0::2, :3], warm[1::2] = ref3["warm_in"][:n], ref5["warm_in"]
    dm = DeviceMooring([ms3, ms5])
    got = dm.eval(r6, sys_idx=idx, warm=warm, jacobian=True, current=U)
    check_eval(got, ref3, slice(0, n), 3, 5, rows=slice(0, None, 2))
    check_eval(got, ref5, slice(None), 5, 5, rows=slice(1, None, 2))


def test_moor_eval_current_flip_geometry():
    """The heavy line of tests/test_mooring.py's ordering flip (U = 3.5 and 4.0 at the zero pose, and
    nearby): along the load the anchor ranks upper, the line is solved fully suspended, the anchor is pulled up."""
    from raft.mooring_device import DeviceMooring
    ms, r6s, U, ref = system_with_reference("flip")
    got = DeviceMooring([ms]).eval(r6s, warm=ref["warm_in"], jacobian=True, current=U)
    check_eval(got, ref, slice(None), 1, 1)
    ln = ms.lines[0]
    ms.current = U[0]
    ms.set_body_positions([r6s[0]])
    assert ln.fA[2] > 0 and ln.pA.r[2] == -ms.depth             # the anchor, on the seabed, is pulled up
    ms.current = np.zeros(3)


def test_current_argument_checks():
    from raft import _native as N
    from raft.mooring_device import DeviceMooring
    ms, r6s, U, _ = system_with_reference("one")
    dm = DeviceMooring([ms])
    with pytest.raises(ValueError, match="non-finite current"):
        dm.eval(r6s, current=np.where(np.arange(3) == 1, np.nan, U))
    with pytest.raises(ValueError, match="expected"):
        dm.eval(r6s, current=U[:-1])
    L = N.lib()
    rc = L.rh_moor_eval_current(N.context(0), dm._arr, N.ptr(dm._arr_dev), 1, 1, None, None, N.ptr(dm._drag), None,
                                *([None] * 7))
    assert rc == N.RH_EINVAL and b"null drag or current" in L.rh_last_error()
    rc = L.rh_statics_solve_current(N.context(0), dm._arr, N.ptr(dm._arr_dev), 1, 1, *([None] * 12))
    assert rc == N.RH_EINVAL and b"null drag or current" in L.rh_last_error()


# ------------------------------------------------------------------------------ statics
def statics_cases():
    return {"current": dict(CASES["current"]), "wave": dict(CASES["wave"]), "seeded": C.seeded_case(CASES["current"], 33)}


_HOST_STATICS = {}


def host_statics(index, key):
    """A fresh currentMod 1 model through solveStatics(case), with its mooring outputs at the offset pose (the
    system's current still set, as analyzeCases reads them)."""
    import raft
    if (index, key) not in _HOST_STATICS:
        m = raft.Model(C.current_design(DESIGNS[index]))
        X = m.solveStatics(dict(statics_cases()[key]))
        ms = m.fowtList[0].ms
        _HOST_STATICS[(index, key)] = dict(
            X=X.copy(), iters=len(m.Xs2), F=ms.body_forces(ms.bodies[0]), K=ms.coupled_stiffness_analytic(),
            T=ms.tensions(), J=ms.coupled_stiffness_fd(tensions=True)[1], current=ms.current.copy())
    return _HOST_STATICS[(index, key)]


@pytest.mark.parametrize("index", [0, 1], ids=DESIGNS)
def test_solve_statics_batch_line_current(index):
    import raft
    from conftest import load_design
    keys = list(statics_cases())
    cases = [dict(statics_cases()[k]) for k in keys]
    m = raft.Model(C.current_design(DESIGNS[index]))
    sb = m.solveStaticsBatch([dict(c) for c in cases], line_current=True)
    assert not sb["status"].any(), sb["status"]
    f = m.fowtList[0]
    np.testing.assert_array_equal(f.r6, [f.x_ref, f.y_ref, 0, 0, 0, 0])      # left at the reference pose
    assert not f.ms.current.any()                                            # ... with no current on the host object
    calm = raft.Model(load_design(DESIGNS[index])).solveStaticsBatch([dict(c) for c in cases])     # currentMod 0
    for i, key in enumerate(keys):
        h = host_statics(index, key)
        assert h["current"].any() == (cases[i]["current_speed"] > 0)
        print(f"{DESIGNS[index]} {key}: |X - X_host| {np.abs(sb['X'][i] - h['X']).max():.2e}, evaluations "
              f"{sb['iters'][i]} / {h['iters']}")
        assert sb["iters"][i] == h["iters"]
        np.testing.assert_allclose(sb["X"][i], h["X"], rtol=1e-9, atol=1e-9)
        errs = dict(C_moor=rel(sb["C_moor"][i], h["K"]), F_moor=rel(sb["F_moor"][i], h["F"]),
                    Tmoor_avg=rel(sb["Tmoor_avg"][i], h["T"]), J_moor=rel(sb["J_moor"][i], h["J"]))
        print("   ", {k: f"{v:.2e}" for k, v in errs.items()})
        assert max(errs.values()) < TOL, errs
        if cases[i]["current_speed"] > 0:
            # the line drag moves the platform further downstream: by more than 0.05 m in the reference's current
            # case, as tests/test_mooring.py::test_mooring_current_moves_the_platform_downstream asserts for the host
            hd = np.radians(cases[i]["current_heading"])
            more = np.dot(sb["X"][i][:2] - calm["X"][i][:2], [np.cos(hd), np.sin(hd)])
            assert more > (0.05 if key == "current" else 0.0), more
            assert np.linalg.norm(sb["X"][i][:2] - calm["X"][i][:2]) < 0.5 * np.linalg.norm(calm["X"][i][:2])
        else:                                  # no current: the bits of the design without currentMod
            for k in sb:
                np.testing.assert_array_equal(sb[k][i], calm[k][i], err_msg=k)
    # with the current loads from the device as well
    sd = m.solveStaticsBatch([dict(c) for c in cases], line_current=True, current_device=True)
    assert np.array_equal(sd["iters"], sb["iters"]) and rel(sd["X"], sb["X"]) < TOL and rel(sd["J_moor"], sb["J_moor"]) < TOL


# ------------------------------------------------------------------------------ dynamics at the offsets
SEA = dict(wave_spectrum="JONSWAP", wave_period=10, wave_height=4, wave_heading=-30)
DYN_CASES = [dict(CASES["wave"]), dict(CASES["current"], wave_period=8, wave_height=2, wave_heading=0),
             dict(CASES["current"], **SEA)]              # tests/test_gpu_moor.py's three shapes


def model40():
    import raft
    d = C.current_design(DESIGNS[0])
    d["settings"].update(min_freq=0.01, max_freq=0.4)
    m = raft.Model(d)
    assert m.nw == 40 and m.mooring_currentMod == 1
    return m


def test_analyze_cases_batch_line_current():
    from raft.fowt import mooring_outputs
    runs = [model40().analyzeCasesBatch([dict(c) for c in DYN_CASES], statics=True, pose_chunk=2, line_current=True, **kw)
            for kw in (dict(), dict(pose_device=True))]
    for res in runs:
        assert not res["statics_status"].any() and np.all(res["status"] >= 0)
    for i, case in enumerate(DYN_CASES):
        mh = model40()
        fh = mh.fowtList[0]
        fh.calcBEM()
        mh.solveStatics(dict(case))
        assert fh.ms.current.any() == (case["current_speed"] > 0)
        Xi = mh.solveDynamics(dict(case))
        out = mooring_outputs(fh.ms, fh._xi_dev, mh.w, mh.device, fh._xi_dev.shape[0])
        for res, name in zip(runs, ("host designs", "pose_device")):
            err = np.linalg.norm(res["Xi"][i] - Xi[0]) / np.linalg.norm(Xi[0])
            print(f"case {i} ({name}): Xi residual {err:.2e}, drag iterations {res['iters'][i]} / {fh.iterations}, "
                  f"statics evaluations {res['statics_iters'][i]} / {len(mh.Xs2)}")
            assert res["iters"][i] == fh.iterations and res["statics_iters"][i] == len(mh.Xs2)
            assert err < TOL
            e_std, e_psd = rel(res["Tmoor_std"][i], out["Tmoor_std"]), rel(res["Tmoor_PSD"][i], out["Tmoor_PSD"])
            print(f"        Tmoor_std {e_std:.2e}, Tmoor_PSD {e_psd:.2e}")
            assert e_std < 1e-8 and e_psd < 1e-8
    a, b = runs
    assert np.array_equal(a["iters"], b["iters"]) and np.array_equal(a["statics_iters"], b["statics_iters"])
    for k in ("Xi", "mean_offsets", "Tmoor_avg", "Tmoor_std", "Tmoor_PSD"):
        assert rel(a[k], b[k]) < TOL, k

"""GPU: the batched mooring evaluation and mean-offset solve (csrc/rh_moor.hip through
raft/mooring_device.py, Model.solveStaticsBatch and analyzeCasesBatch(statics=True)) against the
host MooringSystem / Model.solveStatics / solveDynamics they restate, at the project's device
parity convention (1e-9 of each array's largest entry) and against the reference's own
desired_X0 values at its rtol 1e-5.  Shapes are the smallest that exercise the lane grouping:
3 lines in a group of 4, 4 in 4, 1 in 1, 5 in 8, two systems in one call, and 67 poses (a partial
last wave).  Host references are computed once per module and shared."""
import numpy as np
import pytest

from conftest import load_design
from test_moor_host import CASES, DESIGNS, DESIRED_X0, make_model

pytestmark = pytest.mark.gpu
TOL = 1e-9                       # device parity convention: of each array's largest entry


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max()


# ------------------------------------------------------------------------------ systems
def synthetic(kind):
    """Small systems built with MooringSystem.add_*: "one" (1 line), "four" (4 lines: fills its group)
    and "five" (group of 8) with one line defined vessel-end-first (the swap), one anchor 10 m above
    the seabed (CB < 0) and one taut line."""
    from raft.mooring import MooringSystem, Point
    ms = MooringSystem(depth=200.0)
    ms.add_line_type("chain", 0.15, 350.0, 1.5e9)
    ms.add_line_type("rope", 0.12, 30.0, 2.0e8)
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


def poses(n, seed):
    rng = np.random.default_rng(seed)
    r6 = np.concatenate([rng.uniform(-20, 20, [n, 3]), rng.uniform(-0.1, 0.1, [n, 3])], axis=1)
    r6[:, 2] *= 0.25
    return r6


def host_reference(ms, r6s):
    """F, K, T, J and the warm states before / after each pose on the host system.  Odd poses start
    cold, even poses warm from the pose before (an explicit warm state for the device)."""
    body = ms.bodies[0]
    out = dict(F=[], K=[], T=[], J=[], warm_in=[], warm_out=[])
    for ip, r6 in enumerate(r6s):
        if ip % 2:
            for ln in ms.lines:
                ln.HF = ln.VF = 0.0
        out["warm_in"].append([[ln.HF, ln.VF] for ln in ms.lines])
        ms.set_body_positions([r6])
        out["F"].append(ms.body_forces(body))
        out["K"].append(ms.coupled_stiffness_analytic())
        out["T"].append(ms.tensions())
        out["J"].append(ms.coupled_stiffness_fd(tensions=True)[1])
        out["warm_out"].append([[ln.HF, ln.VF] for ln in ms.lines])
    return {k: np.array(v) for k, v in out.items()}


_CACHE = {}


def system_with_reference(name, n=7):
    if name not in _CACHE:
        ms = make_model(0).fowtList[0].ms if name == "volturn" else synthetic(name)
        r6s = poses(67 if name == "volturn" else n, seed=len(name))
        _CACHE[name] = (ms, r6s, host_reference(ms, r6s))
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
    print("rh_moor_eval residuals", {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) < TOL, errs
    pad = np.setdiff1d(np.arange(2 * nl_max), cols)
    assert not g["T"][:, pad].any() and not g["J"][:, pad].any() and not g["warm"][:, nl:].any()


@pytest.mark.parametrize("n", [1, 5, 67])
def test_moor_eval_volturn(n):
    from raft.mooring_device import DeviceMooring
    ms, r6s, ref = system_with_reference("volturn")
    dm = DeviceMooring([ms])
    assert dm.nl_max == 3
    check_eval(dm.eval(r6s[:n], warm=ref["warm_in"][:n], jacobian=True), ref, slice(0, n), 3, 3)


@pytest.mark.parametrize("kind", ["one", "four", "five"])
def test_moor_eval_synthetic(kind):
    from raft.mooring_device import DeviceMooring
    ms, r6s, ref = system_with_reference(kind)
    nl = len(ms.lines)
    dm = DeviceMooring([ms])
    check_eval(dm.eval(r6s, warm=ref["warm_in"], jacobian=True), ref, slice(None), nl, nl)
    if kind == "five":      # the shapes the system was built for
        from raft.mooring_device import flatten
        tab, depth, _ = flatten(ms)
        assert tab[9].tolist() == [1, 0, 1, 1, 1] and tab[2, 2] > -depth
        assert tab[6, 3] < np.linalg.norm(tab[0:3, 3] - tab[3:6, 3])       # taut at the zero pose
    # without a warm argument every pose starts cold: the odd (cold) host poses
    cold = dm.eval(r6s[1::2], jacobian=True)
    odd = {k: v[1::2] for k, v in ref.items()}
    check_eval(cold, odd, slice(None), nl, nl)


def test_moor_eval_two_systems():
    """nsys = 2 with mixed sys_idx: 3-line and 5-line poses interleaved in one call (groups of 8)."""
    from raft.mooring_device import DeviceMooring
    ms3, r3, ref3 = system_with_reference("volturn")
    ms5, r5, ref5 = system_with_reference("five")
    n = len(r5)
    idx = np.array([0, 1] * n, dtype=np.int32)
    r6 = np.empty([2 * n, 6])
    r6[0::2], r6[1::2] = r3[:n], r5
    warm = np.zeros([2 * n, 5, 2])
    warm[0::2, :3], warm[1::2] = ref3["warm_in"][:n], ref5["warm_in"]
    dm = DeviceMooring([ms3, ms5])
    got = dm.eval(r6, sys_idx=idx, warm=warm, jacobian=True)
    check_eval(got, ref3, slice(0, n), 3, 5, rows=slice(0, None, 2))
    check_eval(got, ref5, slice(None), 5, 5, rows=slice(1, None, 2))


# ------------------------------------------------------------------------------ statics
_HOST_STATICS = {}


def host_statics(index, key):
    """A fresh model through solveStatics(case), with its mooring outputs at the offset pose."""
    if (index, key) not in _HOST_STATICS:
        m = make_model(index, aero=key.startswith("wind"))
        X = m.solveStatics(dict(CASES[key]))
        ms = m.fowtList[0].ms
        _HOST_STATICS[(index, key)] = dict(
            X=X.copy(), iters=len(m.Xs2), F=ms.body_forces(ms.bodies[0]), K=ms.coupled_stiffness_analytic(),
            T=ms.tensions(), J=ms.coupled_stiffness_fd(tensions=True)[1])
    return _HOST_STATICS[(index, key)]


@pytest.mark.parametrize("index", [0, 1], ids=DESIGNS)
@pytest.mark.parametrize("keys", [("wave", "current"), ("wind", "wind_wave_current")], ids=["plain", "aero"])
def test_solve_statics_batch(index, keys):
    m = make_model(index, aero=keys[0].startswith("wind"))
    sb = m.solveStaticsBatch([dict(CASES[k]) for k in keys])
    assert not sb["status"].any(), sb["status"]
    f = m.fowtList[0]
    np.testing.assert_array_equal(f.r6, [f.x_ref, f.y_ref, 0, 0, 0, 0])      # left at the reference pose
    for i, key in enumerate(keys):
        np.testing.assert_allclose(sb["X"][i], DESIRED_X0[key][index], rtol=1e-5, atol=1e-10)
        h = host_statics(index, key)
        print(f"{DESIGNS[index]} {key}: |X - X_host| {np.abs(sb['X'][i] - h['X']).max():.2e}, evaluations "
              f"{sb['iters'][i]} / {h['iters']}")
        assert sb["iters"][i] == h["iters"]
        np.testing.assert_allclose(sb["X"][i], h["X"], rtol=1e-9, atol=1e-9)
        np.testing.assert_array_equal(sb["Xi0"][i], sb["X"][i] - np.array([f.x_ref, f.y_ref, 0, 0, 0, 0]))
        errs = dict(C_moor=rel(sb["C_moor"][i], h["K"]), F_moor=rel(sb["F_moor"][i], h["F"]),
                    Tmoor_avg=rel(sb["Tmoor_avg"][i], h["T"]), J_moor=rel(sb["J_moor"][i], h["J"]))
        print("   ", {k: f"{v:.2e}" for k, v in errs.items()})
        assert max(errs.values()) < TOL, errs


def test_solve_statics_batch_row_is_independent_of_its_neighbours():
    """67 copies of the current case with seeded speeds: row 0 equals the single-case result bit for
    bit (a case does not depend on the cases in the lanes next to it)."""
    rng = np.random.default_rng(67)
    cases = [dict(CASES["current"], current_speed=float(s)) for s in rng.uniform(0.0, 1.0, 67)]
    m = make_model(0)
    many = m.solveStaticsBatch(cases)
    one = m.solveStaticsBatch(cases[:1])
    assert not many["status"].any()
    assert len(np.unique(many["iters"])) > 1 or many["iters"][0] > 1
    for k in one:
        np.testing.assert_array_equal(many[k][0], one[k][0], err_msg=k)
    # and the rows are the cases' own: the offset grows with the current speed (the slowest currents
    # stay within the Newton's first-step tolerance of the reference pose)
    speeds = np.array([c["current_speed"] for c in cases])
    off = np.hypot(many["X"][:, 0], many["X"][:, 1])[np.argsort(speeds)]
    assert np.all(np.diff(off) >= 0) and off[-1] > off[0] + 1.0


def test_statics_argument_checks():
    from raft import _native as N
    from raft.mooring_device import DeviceMooring
    ms, r6s, _ = system_with_reference("one")
    dm = DeviceMooring([ms])
    with pytest.raises(ValueError):
        dm.eval(r6s, sys_idx=np.ones(len(r6s), dtype=np.int32))
    arr = (N.RhMoorSystem * 1)()
    arr[0].nline, arr[0].tol, arr[0].line = 65, 1e-5, dm._tables[0].data_ptr()
    rc = N.lib().rh_moor_eval(N.context(0), arr, N.ptr(dm._arr_dev), 1, 1, *([None] * 9))
    assert rc == N.RH_EINVAL and b"nline=65" in N.lib().rh_last_error()


# ------------------------------------------------------------------------------ dynamics at the offsets
# Three no-wind cases: the reference's `wave` case, its `current` case, and one with both.  The
# `current` case as the reference holds it has wave_period 0 and wave_height 0, for which the JONSWAP
# spectrum is 0/0 on the host and the device alike (solveDynamics raises "Nan detected"), so here it
# carries a small sea of its own: the response needs one.
SEA = dict(wave_spectrum="JONSWAP", wave_period=10, wave_height=4, wave_heading=-30)
DYN_CASES = [dict(CASES["wave"]), dict(CASES["current"], wave_period=8, wave_height=2, wave_heading=0),
             dict(CASES["current"], **SEA)]


def model40():
    import raft
    d = load_design(DESIGNS[0])
    d["settings"].update(min_freq=0.01, max_freq=0.4)
    m = raft.Model(d)
    assert m.nw == 40
    return m


def test_analyze_cases_batch_with_statics():
    from raft.fowt import mooring_outputs
    m = model40()
    res = m.analyzeCasesBatch([dict(c) for c in DYN_CASES], statics=True, pose_chunk=2)
    assert not res["statics_status"].any() and np.all(res["status"] >= 0)
    sb = model40().solveStaticsBatch([dict(c) for c in DYN_CASES])      # (a model as fresh as `m` was)
    np.testing.assert_array_equal(res["mean_offsets"], sb["X"])
    np.testing.assert_array_equal(res["Tmoor_avg"], sb["Tmoor_avg"])
    for i, case in enumerate(DYN_CASES):
        mh = model40()
        fh = mh.fowtList[0]
        fh.calcBEM()
        mh.solveStatics(dict(case))
        Xi = mh.solveDynamics(dict(case))
        err = np.linalg.norm(res["Xi"][i] - Xi[0]) / np.linalg.norm(Xi[0])
        print(f"case {i}: Xi residual {err:.2e}, drag iterations {res['iters'][i]} / {fh.iterations}, statics "
              f"evaluations {res['statics_iters'][i]} / {len(mh.Xs2)}")
        assert res["iters"][i] == fh.iterations and res["statics_iters"][i] == len(mh.Xs2)
        assert err < TOL
        out = mooring_outputs(fh.ms, fh._xi_dev, mh.w, mh.device, fh._xi_dev.shape[0])
        e_std, e_psd = rel(res["Tmoor_std"][i], out["Tmoor_std"]), rel(res["Tmoor_PSD"][i], out["Tmoor_PSD"])
        print(f"        Tmoor_std {e_std:.2e}, Tmoor_PSD {e_psd:.2e}")
        assert e_std < 1e-8 and e_psd < 1e-8


def test_analyze_cases_batch_without_statics_is_unchanged():
    m = model40()
    cases = [dict(c) for c in DYN_CASES]
    a = m.analyzeCasesBatch([dict(c) for c in cases])
    b = m.analyzeCasesBatch([dict(c) for c in cases], statics=False)
    assert set(a) == set(b) and "mean_offsets" not in a
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_statics_keyword_refusals():
    import raft
    from conftest import load_golden, statics_of
    m = model40()
    m.fowtList[0].potSecOrder = 1
    with pytest.raises(NotImplementedError, match="potSecOrder"):
        m.analyzeCasesBatch([dict(CASES["wave"])], statics=True)
    T = load_golden("c1_OC3spar")
    mf = raft.Model(load_design("OC3spar"), statics=[statics_of(T)])
    with pytest.raises(NotImplementedError):
        mf.analyzeCasesBatch([dict(CASES["wave"])], statics=True)

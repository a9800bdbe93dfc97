"""GPU parity of designs with potential-flow coefficient files (potFirstOrder = 1): the
rh_bem_excitation kernel against a NumPy restatement, F_BEM and the response solve against the
reference runs of tests/golden/bem_*.npz (make_bem_golden.py), and every consumer of the
excitation table (solveDynamics, analyzeCasesBatch, DesignBatch, analyzeArrayBatch, the sharded
entry points) on such a design.  nw = 20 throughout the model tests."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, farm_tables, golden_cases, load_design, load_golden, statics_of

pytestmark = pytest.mark.gpu
RTOL = 1e-9                      # tests/test_gpu_parity.py: FP64, normwise per case
BEM = os.path.join(GOLDEN, "bem")
GRID = dict(min_freq=0.02, max_freq=0.4)
DOFS = ["surge", "sway", "heave", "roll", "pitch", "yaw"]
FIXTURES = {"bem_a": ("Buoy", 1), "bem_b": ("synth", 3), "bem_c": ("synth_unsorted", 3)}


def rel(a, b):
    nb = np.linalg.norm(b)
    return np.linalg.norm(a - b) / (nb if nb > 0 else 1.0)


def bem_design(hydro, master, base="OC3spar"):
    d = load_design(base)
    d["settings"].update(GRID)
    d["platform"].update(potFirstOrder=1, potModMaster=master, hydroPath=os.path.join(BEM, hydro))
    return d


_MODELS = {}


def model_of(tag):
    """One model per fixture for the whole module (its device tables are reused by the tests)."""
    if tag not in _MODELS:
        import raft
        T = load_golden(tag)
        hydro, master = FIXTURES[tag]
        m = raft.Model(bem_design(hydro, master), statics=[statics_of(T)])
        f = m.fowtList[0]
        f.setPosition(T["r6"])
        f.calcStatics()
        f.calcBEM()
        f.calcHydroConstants()
        _MODELS[tag] = (m, f, T, golden_cases(T))
    return _MODELS[tag]


def ref_of(T, key, ic):
    return T[f"out_{key}_{ic}"] if f"out_{key}_{ic}" in T else T["out_" + key][ic]


# ---------------------------------------------------------------------------- the kernel alone
def numpy_bem(k, hd, X, beta, hadj, x_ref, y_ref, finer):
    """FOWT.calcHydroExcitation's F_BEM block (raft/raft_fowt.py:1041-1093) per unit amplitude."""
    nh, nw = len(beta), len(k)
    fbem = np.zeros([nh, 6, nw], dtype=complex)
    nhs = len(hd)
    for ih in range(nh):
        phase = np.exp(-1j * k * (x_ref * np.cos(beta[ih]) + y_ref * np.sin(beta[ih])))
        b = (np.degrees(beta[ih]) - hadj) % 360
        if b <= hd[0]:
            hlast = hd[-1] - 360
            i1, i2 = nhs - 1, 0
            f2 = (b - hlast) / (hd[0] - hlast)
        elif b >= hd[nhs - 1]:
            hfirst = hd[0] + 360
            i1, i2 = nhs - 1, 0
            f2 = (b - hd[-1]) / (hfirst - hd[-1])
        else:
            for i in range(nhs - 1):
                if hd[i + 1] > b:
                    i1, i2 = i, i + 1
                    f2 = (b - hd[i]) / (hd[i + 1] - hd[i])
                    break
        f1 = 1.0 - f2
        Xp = X[i1] * f1 + X[i2] * f2
        s, c = np.sin(beta[ih]), np.cos(beta[ih])
        Xg = np.zeros([6, nw], dtype=complex)
        Xg[0] = Xp[0] * c - Xp[1] * s
        Xg[1] = Xp[0] * s + Xp[1] * c
        Xg[2] = Xp[2]
        Xg[3] = Xp[3] * c - Xp[4] * s
        Xg[4] = Xp[3] * s + Xp[4] * c
        Xg[5] = Xp[5]
        fbem[ih] = Xg * phase
    return fbem, finer + fbem


def run_kernel(k, hd, X, beta, hadj, x_ref, y_ref, finer):
    import torch
    from raft import _native as N
    dev = torch.device("cuda", 0)
    t = lambda a, dt: torch.tensor(np.ascontiguousarray(a), dtype=dt, device=dev)   # noqa: E731
    kt, ht, bt = t(k, torch.float64), t(hd, torch.float64), t(beta, torch.float64)
    Xt, ft = t(X, torch.complex128), t(finer, torch.complex128)
    fb, fx = torch.full_like(ft, float("nan")), torch.full_like(ft, float("nan"))
    N.check(N.lib().rh_bem_excitation(N.context(0), len(k), N.ptr(kt), len(hd), N.ptr(ht), N.ptr(Xt), len(beta), N.ptr(bt),
                                      float(hadj), float(x_ref), float(y_ref), N.ptr(ft), N.ptr(fb), N.ptr(fx),
                                      N.stream_handle(torch, dev)), "rh_bem_excitation")
    return fb.cpu().numpy(), fx.cpu().numpy()


KERNEL_SHAPES = {
    # name: (nw, BEM headings [deg], output headings [deg], heading_adjust, x_ref, y_ref)
    "odd_grid": (37, [0.0, 90.0, 180.0, 270.0], [12.0, 200.0], 0.0, 0.0, 0.0),
    "single_heading": (20, [30.0], [40.0], 0.0, 0.0, 0.0),                       # i1 = i2 = 0
    "single_heading_below": (20, [30.0], [10.0, 30.0], 0.0, 0.0, 0.0),
    "three_headings": (20, [10.0, 120.0, 250.0], [0.0, 10.0, 250.0, 359.5, 120.0, 119.0], 0.0, 0.0, 0.0),
    "array_position": (300, [0.0, 90.0, 180.0, 270.0], [45.0, 180.0, 300.0], 25.0, 800.0, -350.0),   # two blocks of bins
    "negative_heading": (64, [0.0, 90.0, 180.0, 270.0], [-30.0, 360.0, 725.0], 100.0, -60.0, 10.0),
}


@pytest.mark.parametrize("name", list(KERNEL_SHAPES))
def test_kernel_matches_numpy_restatement(name):
    nw, hd, betas, hadj, x_ref, y_ref = KERNEL_SHAPES[name]
    rng = np.random.default_rng(7)
    k = np.linspace(0.002, 0.7, nw)
    X = rng.normal(size=[len(hd), 6, nw]) * 1e6 + 1j * rng.normal(size=[len(hd), 6, nw]) * 1e6
    beta = np.deg2rad(np.array(betas))
    finer = rng.normal(size=[len(betas), 6, nw]) * 1e5 + 1j * rng.normal(size=[len(betas), 6, nw]) * 1e5
    fb, fx = run_kernel(k, np.array(hd), X, beta, hadj, x_ref, y_ref, finer)
    rb, rx = numpy_bem(k, np.array(hd), X, beta, hadj, x_ref, y_ref, finer)
    eb = np.max(np.abs(fb - rb)) / np.max(np.abs(rb))
    ex = np.max(np.abs(fx - rx)) / np.max(np.abs(rx))
    print(f"{name}: fbem {eb:.2e} fexc {ex:.2e}")
    assert eb < 1e-13 and ex < 1e-13            # double-precision rounding of a dozen operations


def test_kernel_rejects_bad_arguments():
    import torch
    from raft import _native as N
    z = torch.zeros(6 * 4, dtype=torch.complex128, device="cuda:0")
    r = torch.zeros(4, dtype=torch.float64, device="cuda:0")
    s = N.stream_handle(torch, torch.device("cuda", 0))
    L, ctx = N.lib(), N.context(0)
    assert L.rh_bem_excitation(ctx, 4, N.ptr(r), 0, N.ptr(r), N.ptr(z), 1, N.ptr(r), 0.0, 0.0, 0.0, N.ptr(z),
                               N.ptr(z.clone()), N.ptr(z.clone()), s) == N.RH_EINVAL          # nhb = 0
    assert L.rh_bem_excitation(ctx, 4, N.ptr(r), 1, N.ptr(r), N.ptr(z), 1, N.ptr(r), 0.0, 0.0, 0.0, N.ptr(z),
                               N.ptr(z.clone()), N.ptr(z), s) == N.RH_EINVAL                  # fexc aliases finer
    assert L.rh_bem_excitation(ctx, 4, N.ptr(r), 1, N.ptr(r), None, 1, N.ptr(r), 0.0, 0.0, 0.0, N.ptr(z),
                               N.ptr(z.clone()), N.ptr(z.clone()), s) == N.RH_EINVAL          # null X


# ---------------------------------------------------------------------------- F_BEM
@pytest.mark.parametrize("tag", ["bem_b", "bem_c"])
def test_f_bem_matches_reference(tag):
    m, f, T, cases = model_of(tag)
    for ic, case in enumerate(cases):
        f.calcHydroExcitation(dict(case), memberList=f.memberList)
        ref = ref_of(T, "F_BEM", ic)
        assert f.F_BEM.shape == ref.shape
        assert np.abs(ref).max() > 1e3
        assert rel(f.F_BEM, ref) < RTOL, (ic, rel(f.F_BEM, ref))
        assert rel(f.F_hydro_iner, ref_of(T, "F_iner", ic)) < RTOL
        assert not f.F_hydro_iner.any()                   # potModMaster 3: no strip-theory inertia at all


def test_f_bem_of_a_fowt_in_an_array_matches_reference():
    """(d): x_ref = 30, y_ref = -20, heading_adjust = 25 and readHydro's unsorted tables, four sea
    states in one call: below the first file heading after the adjustment, on it, inside, above."""
    import raft
    from raft.fowt import FOWT
    T = load_golden("bem_d")
    d = bem_design("synth", 0)
    f = FOWT(d, raft.Model.frequency_grid(d), None, depth=float(d["site"]["water_depth"]), x_ref=float(T["x_ref"]),
             y_ref=float(T["y_ref"]), heading_adjust=float(T["heading_adjust"]))
    f.setStatics(statics_of(T))
    f.setPosition(T["r6"])
    f.calcStatics()
    f.calcHydroConstants()
    case = golden_cases(T)[0]
    f.calcHydroExcitation(dict(case), memberList=f.memberList)
    assert f.F_BEM.shape == T["out_F_BEM"].shape == (4, 6, 20)
    assert rel(f.F_BEM, T["out_F_BEM"]) < RTOL, rel(f.F_BEM, T["out_F_BEM"])
    for ih in range(4):
        assert rel(f.F_BEM[ih], T["out_F_BEM"][ih]) < RTOL
    assert rel(f.F_hydro_iner, T["out_F_iner"]) < RTOL


def test_pot_mod_master_1_has_tables_but_no_f_bem():
    m, f, T, cases = model_of("bem_a")
    f.calcHydroExcitation(dict(cases[0]), memberList=f.memberList)
    assert not f.F_BEM.any() and not ref_of(T, "F_BEM", 0).any()
    assert f.device_design().bem is None and f.device_design().per_bin
    assert rel(f.F_hydro_iner, ref_of(T, "F_iner", 0)) < RTOL


# ---------------------------------------------------------------------------- the response solve
@pytest.mark.parametrize("tag", list(FIXTURES))
def test_solve_dynamics_matches_reference(tag):
    m, f, T, cases = model_of(tag)
    for ic, case in enumerate(cases):
        Xi = m.solveDynamics(dict(case))
        ref = ref_of(T, "Xi", ic)
        assert f.iterations == T["out_iters"][ic], (ic, f.iterations, T["out_iters"][ic])
        assert int(f.converged) == T["out_conv"][ic]
        assert Xi.shape == ref.shape
        for row in range(Xi.shape[0] - 1):                      # every sea state's response
            assert rel(Xi[row], ref[row]) < RTOL, (ic, row, rel(Xi[row], ref[row]))
        assert not Xi[-1].any()
        assert rel(f.Z, T["out_Z"][ic]) < 1e-12, rel(f.Z, T["out_Z"][ic])
        assert rel(f.B_hydro_drag, T["out_B_drag"][ic]) < RTOL
        res = {}
        f.saveTurbineOutputs(res, case)
        std, psd = T["out_std"][ic], T["out_PSD"][ic]
        for j, dof in enumerate(DOFS):
            np.testing.assert_allclose(res[dof + "_std"], std[j], rtol=RTOL, atol=RTOL * std.max())
            np.testing.assert_allclose(res[dof + "_PSD"], psd[j], rtol=RTOL, atol=RTOL * psd.max())


def test_analyze_cases_runs_a_bem_design():
    """analyzeCases (calcBEM inside, potModMaster 3) and calcOutputs on a BEM design: the case
    metrics of (c)'s case equal the reference's motion statistics."""
    import raft
    T = load_golden("bem_c")
    d = bem_design("synth_unsorted", 3)
    case = golden_cases(T)[0]
    keys = ["wind_speed", "wind_heading", "turbulence", "turbine_status", "yaw_misalign", "wave_spectrum", "wave_period",
            "wave_height", "wave_heading", "wave_gamma"]
    full = {**dict(wind_speed=0, wind_heading=0, turbulence=0, turbine_status="operating", yaw_misalign=0), **case}
    d["cases"] = {"keys": keys, "data": [[full[k] for k in keys]]}
    m = raft.Model(d, statics=[statics_of(T)])
    r = m.analyzeCases()
    m.calcOutputs()
    assert list(m.fowtList[0].BEM_headings) == [0.0, 90.0, 180.0, 270.0]
    got = np.array([r["case_metrics"][0][0][dof + "_std"] for dof in DOFS])
    np.testing.assert_allclose(got, T["out_std"][0], rtol=RTOL, atol=RTOL * T["out_std"][0].max())


def test_batches_equal_solve_dynamics():
    """analyzeCasesBatch on (b)'s cases (the two-sea-state one included) and DesignBatch.solve with
    full models (a BEM design next to a strip-theory one: one batched table launch for both)
    against Model.solveDynamics, at the bound of test_multi_sea_state_cases_through_the_batch."""
    import raft
    from raft.batch import DesignBatch
    m, f, T, cases = model_of("bem_b")
    res = m.analyzeCasesBatch([dict(c) for c in cases])
    np.testing.assert_array_equal(res["nWaves"], [2, 1, 1])
    singles = []
    for ic, case in enumerate(cases):
        Xi = m.solveDynamics(dict(case))
        nW = Xi.shape[0] - 1
        assert res["iters"][ic] == f.iterations == T["out_iters"][ic]
        assert rel(res["Xi_waves"][ic, :nW + 1], Xi) < 1e-12, ic
        assert rel(res["Xi"][ic], Xi[0]) < 1e-12, ic
        assert rel(res["Xi"][ic], ref_of(T, "Xi", ic)[0]) < RTOL
        np.testing.assert_allclose(res["std"][ic], f._stats["std"], rtol=1e-12, atol=1e-15)
        if nW == 1:
            singles.append((dict(case), Xi[0].copy(), f.iterations))
    Ta = load_golden("c1_OC3spar")
    plain = load_design("OC3spar")
    plain["settings"].update(GRID)
    mp = raft.Model(plain, statics=[statics_of(Ta)])
    fp = mp.fowtList[0]
    fp.setPosition(Ta["r6"])
    fp.calcStatics()
    fp.calcHydroConstants()
    B = DesignBatch([bem_design("synth", 3), plain], statics=[statics_of(T), statics_of(Ta)])
    assert B.dds[0].bem is not None and B.dds[1].bem is None
    bc = [c for c, _, _ in singles]
    h = B.solve(np.array([0] * len(bc) + [1] * len(bc)), bc + bc).host()
    for i, (case, Xi0, its) in enumerate(singles):
        assert h["iters"][i] == its
        assert rel(h["Xi"][i], Xi0) < 1e-12, i
        Xp = mp.solveDynamics(dict(case))
        assert h["iters"][len(bc) + i] == fp.iterations
        assert rel(h["Xi"][len(bc) + i], Xp[0]) < 1e-12, i
    assert B.dds[1].struct().finer == B.dds[1]._tab_ptr("finer").value
    assert B.dds[0].struct().finer == B.dds[0]._tab_ptr("fexc").value


def test_array_batch_matches_reference():
    """(e): the two-FOWT coupled farm, both platforms on the synthetic files (potModMaster 3),
    heading_adjust 180 / 0 and x = 0 / 1600 m: analyzeArrayBatch and solveDynamics against the
    reference's system response."""
    import raft
    T = load_golden("bem_e")
    Ts = farm_tables(T)
    d = load_design("VolturnUS-S_farm")
    d["settings"].update(GRID)
    for key in ("platform", "platforms"):
        ps = d.get(key)
        for p in (ps if isinstance(ps, list) else [ps] if ps else []):
            p.update(potFirstOrder=1, potModMaster=3, hydroPath=os.path.join(BEM, "synth"))
    m = raft.Model(d, statics=[statics_of(t) for t in Ts])
    m.K_array = T["K_array"]
    for f, t in zip(m.fowtList, Ts):
        f.setPosition(t["r6"])
        f.calcStatics()
        f.calcHydroConstants()
    case = golden_cases(T)[0]
    r = m.analyzeCasesBatch([dict(case)])
    assert list(r["iters"][0]) == list(T["out_iters"])
    assert rel(r["Xi"][0], T["out_Xi"][0]) < RTOL, rel(r["Xi"][0], T["out_Xi"][0])
    Xi = m.solveDynamics(dict(case))
    assert [f.iterations for f in m.fowtList] == list(T["out_iters"])
    assert rel(Xi, T["out_Xi"]) < RTOL, rel(Xi, T["out_Xi"])
    for i, f in enumerate(m.fowtList):
        assert rel(f.F_BEM, T["out_F_BEM"][i]) < RTOL


# ---------------------------------------------------------------------------- isolation and tables
def test_no_table_leaks_between_designs():
    """A strip-theory design solved before and after a BEM design in the same process gives the
    same bits, and its descriptor never points at a BEM table."""
    import raft
    Ta = load_golden("c1_OC3spar")

    def plain():
        d = load_design("OC3spar")
        d["settings"].update(GRID)
        mp = raft.Model(d, statics=[statics_of(Ta)])
        fp = mp.fowtList[0]
        fp.setPosition(Ta["r6"])
        fp.calcStatics()
        fp.calcHydroConstants()
        return mp, fp
    case = dict(wave_spectrum=["JONSWAP"] * 2, wave_period=[9.0, 12.0], wave_height=[4.0, 2.0], wave_heading=[30.0, 200.0],
                wave_gamma=[0.0, 0.0])
    mp, fp = plain()
    before = mp.solveDynamics(dict(case)).copy()
    dd = fp.device_design()
    assert dd.bem is None and dd.fexc is None and dd.struct().finer == dd.finer.data_ptr()
    m, f, T, cases = model_of("bem_b")
    m.solveDynamics(dict(cases[0]))
    after_same = mp.solveDynamics(dict(case))
    mq, fq = plain()
    after_new = mq.solveDynamics(dict(case))
    np.testing.assert_array_equal(before, after_same)
    np.testing.assert_array_equal(before, after_new)
    assert not fq.F_BEM.any()


def test_retabulate_leaves_fexc_bit_equal():
    m, f, T, cases = model_of("bem_b")
    f.calcHydroExcitation(dict(cases[0]), memberList=f.memberList)
    dd = f.device_design()
    assert dd.struct().finer == dd.fexc.data_ptr() != dd.finer.data_ptr()
    fexc, fbem, finer = dd.fexc.clone(), dd.fbem.clone(), dd.finer.clone()
    assert rel((fexc - finer).cpu().numpy(), fbem.cpu().numpy()) < 1e-15
    dd.fexc.fill_(float("nan"))
    dd.retabulate()
    assert bool((dd.fexc == fexc).all()) and bool((dd.fbem == fbem).all()) and bool((dd.finer == finer).all())


# ---------------------------------------------------------------------------- sharded entry points
def test_sharded_entry_points_carry_the_bem_tables():
    """raft/parallel.py takes the design through its descriptor (per-bin M and B, `finer` at fexc):
    the case-sharded and the bin-sharded solve of a BEM design reproduce the reference run."""
    from raft.parallel import solve_bins_sharded, solve_cases_sharded
    from raft.solver import CaseSet
    m, f, T, cases = model_of("bem_b")
    single = [(ic, c) for ic, c in enumerate(cases) if np.isscalar(c["wave_heading"])]
    cs = CaseSet([0] * len(single), [c["wave_heading"] for _, c in single], ["JONSWAP"] * len(single),
                 [c["wave_height"] for _, c in single], [c["wave_period"] for _, c in single],
                 [c["wave_gamma"] for _, c in single])
    res, _ = solve_cases_sharded([f.device_design()], cs, m.nIter, m.XiStart, want=("std",))
    for j, (ic, c) in enumerate(single):
        assert int(res["iters"][j]) == T["out_iters"][ic]
        assert rel(res["Xi"][j].cpu().numpy(), ref_of(T, "Xi", ic)[0]) < RTOL
        Xi, iters, status, Bd = solve_bins_sharded(f, dict(c), m.nIter, m.XiStart, shards=[(0, 7), (7, 20)])
        assert iters == T["out_iters"][ic]
        assert rel(Xi, ref_of(T, "Xi", ic)[0]) < RTOL, rel(Xi, ref_of(T, "Xi", ic)[0])

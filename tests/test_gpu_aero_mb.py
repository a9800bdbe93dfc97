"""GPU: aero-servo added mass and damping of batched wind cases on the device (csrc/rh_aero.hip
through raft/rotor_device.py, FOWT.aeroMBBatch and the aero_device= keyword of analyzeCasesBatch)
against the host build of the same header (tools/aero_host.cpp, which tests/test_aero_host.py ties to
the Python) and against the host paths they replace.

Shapes of the entry check: nw = 1, 63, 64, 65 and 200 (one bin, both sides of a wave, two 128-bin
tiles with a partial one) times 1, 3 and 67 cases; modes 1 and 2 mixed in one launch, a case without
a pair between two with pairs, two pairs on one case; constant and per-bin base.  The pair inputs are
those of the CPU test (VolturnUS-S_aero at the schedule speeds, computed once per module) and its
synthetic two-pair table."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import load_design

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import aero_cases as AC  # noqa: E402

pytestmark = pytest.mark.gpu

from test_aero_host import AERO_TERM_BAR  # noqa: E402  (the aero term's bar, measured on the CPU there)

# Measured on the device (MI355X): the normwise relative difference of Xi between
# analyzeCasesBatch(aero_device=True) and analyzeCasesBatch(rotor_device=True) over the four wind
# cases: 6.10e-16 with aeroServoMod 1, 1.25e-13 with aeroServoMod 2 (whose added mass, up to 5e11 at the
# lowest bins, dwarfs the structure's, so that roundings of M at the 8 eps level show in the response).
# Each mode is asserted at ten times its own figure, and never above 1e-9.  (For scale:
# rotor_device=True against the host rotor measured 1.73e-13.)
XI_MEASURED = {1: 6.10e-16, 2: 1.25e-13}
XI_BAR = {mod: min(10 * v, 1e-9) for mod, v in XI_MEASURED.items()}

NWS = [1, 63, 64, 65, 200]
NCASES = [1, 3, 67]
FIVE = [AC.wind_case(4, 0.0), AC.wind_case(10.59, 20.0), AC.wind_case(14, 0.0), AC.wind_case(24, 20.0),
        dict(AC.wind_case(30, 0.0), turbine_status="parked")]


@pytest.fixture(scope="module")
def lib():
    return AC.host_lib()


@pytest.fixture(scope="module")
def pool():
    """The pairs the launches draw from: VolturnUS-S_aero with aeroServoMod 2 and 1 at the five
    schedule speeds (heading 20 deg, the posed platform), then the two synthetic pairs."""
    rows = []
    for mod in (2, 1):
        fowt = AC.posed_model(mod).fowtList[0]
        for U in AC.SPEEDS:
            pin = AC.pair_inputs(fowt, AC.wind_case(U, 20.0))
            rows.append((pin["loads"], pin["dloads"], pin["param"], pin["mode"]))
    loads, dloads, param, modes = AC.synthetic_pairs()
    rows += [(loads[p], dloads[p], param[p], modes[p]) for p in (0, 1)]
    return rows


def layout(ncase, pool):
    """pair_case and the pool index of every pair: case 0 one real pair (mode 2), case 1 none, case 2
    the two synthetic pairs (modes 2 and 1), then the pool in turn, every fifth case without a pair
    and every seventh with two."""
    n = len(pool)
    per_case = [[0], [], [n - 2, n - 1]]
    for c in range(3, ncase):
        per_case.append([] if c % 5 == 0 else ([c % n, (3 * c) % n] if c % 7 == 0 else [c % n]))
    per_case = per_case[:ncase]
    pair_case = [c for c, ps in enumerate(per_case) for _ in ps]
    picks = [p for ps in per_case for p in ps]
    return pair_case, picks


def tables(pool, picks):
    return (np.array([pool[p][0] for p in picks]), np.array([pool[p][1] for p in picks]),
            np.array([pool[p][2] for p in picks]), [pool[p][3] for p in picks])


def grid(nw):
    return np.array([0.5]) if nw == 1 else np.linspace(0.03, 1.3, nw)


def bases(nw, per_bin):
    rng = np.random.default_rng(100 + nw)
    shape = [nw, 6, 6] if per_bin else [6, 6]
    return rng.normal(size=shape) * 1e8, rng.normal(size=shape) * 1e7


def device_mb(ncase, pair_case, modes, loads, dloads, param, w, M0, B0):
    """rh_rotor_aero_mb on device copies of host tables: M, B, f_aero0 as NumPy arrays."""
    import torch
    from raft import _native as N
    dev = torch.device("cuda:0")
    f64 = dict(dtype=torch.float64, device=dev)
    pc, md = np.ascontiguousarray(pair_case, dtype=np.int32), np.ascontiguousarray(modes, dtype=np.int32)
    t = {k: torch.tensor(np.ascontiguousarray(v, dtype=float), **f64) for k, v in
         dict(loads=loads, dloads=dloads, param=param, w=w, M0=M0, B0=B0).items()}
    pcd = torch.tensor(pc, dtype=torch.int32, device=dev)
    nw = len(w)
    M, B = torch.full([ncase, nw, 6, 6], np.nan, **f64), torch.full([ncase, nw, 6, 6], np.nan, **f64)
    f0 = torch.full([ncase, 6], np.nan, **f64)
    N.check(N.lib().rh_rotor_aero_mb(N.context(0), ncase, len(pc), nw, N.ptr(t["w"]), N.ptr(pcd), pc.ctypes.data,
                                     md.ctypes.data, N.ptr(t["loads"]), N.ptr(t["dloads"]), N.ptr(t["param"]),
                                     N.ptr(t["M0"]), N.ptr(t["B0"]), int(np.ndim(M0) == 3), N.ptr(M), N.ptr(B), N.ptr(f0),
                                     N.stream_handle(torch, dev)), "rh_rotor_aero_mb")
    torch.cuda.synchronize()
    return M.cpu().numpy(), B.cpu().numpy(), f0.cpu().numpy()


@pytest.fixture(scope="module")
def launches(pool):
    """(nw, ncase, per_bin) -> the device's (M, B, f0), launched once and shared."""
    out = {}

    def get(nw, ncase, per_bin):
        key = (nw, ncase, per_bin)
        if key not in out:
            pair_case, picks = layout(ncase, pool)
            loads, dloads, param, modes = tables(pool, picks)
            M0, B0 = bases(nw, per_bin)
            out[key] = device_mb(ncase, pair_case, modes, loads, dloads, param, grid(nw), M0, B0)
        return out[key]
    return get


# ------------------------------------------------------------------------------ the entry against the header
@pytest.mark.parametrize("ncase", NCASES)
@pytest.mark.parametrize("nw", NWS)
def test_entry_against_the_host_header(lib, pool, launches, nw, ncase):
    """Every case's M and B within 8 eps max|entry| of the bin's matrix (the CPU test's derived bar), the
    aero term alone (zero base) and f_aero0 to the aero term's bar, every output written (no NaN left
    of the fill), a case without a pair equal to the base bit for bit."""
    pair_case, picks = layout(ncase, pool)
    loads, dloads, param, modes = tables(pool, picks)
    w = grid(nw)
    assert {1, 2} <= set(modes) or ncase == 1
    Z = np.zeros([6, 6])
    hA, hB, hf = AC.host_mb(lib, ncase, pair_case, modes, loads, dloads, param, w, Z, Z)
    dA, dB, df = device_mb(ncase, pair_case, modes, loads, dloads, param, w, Z, Z)
    with_pair = sorted(set(pair_case))
    for c in range(ncase):
        if c in with_pair:
            for got, want in ((dA[c], hA[c]), (dB[c], hB[c]), (df[c], hf[c])):
                assert AC.term_error(got, want) <= AERO_TERM_BAR, (c, AC.term_error(got, want))
        else:
            assert not np.any(dA[c]) and not np.any(dB[c]) and not np.any(df[c])
    for per_bin in (False, True):
        M0, B0 = bases(nw, per_bin)
        hM, hBb, hf = AC.host_mb(lib, ncase, pair_case, modes, loads, dloads, param, w, M0, B0)
        dM, dBb, df = launches(nw, ncase, per_bin)
        assert np.all(np.isfinite(dM)) and np.all(np.isfinite(dBb)) and np.all(np.isfinite(df))
        for c in range(ncase):
            if c not in with_pair:
                assert np.array_equal(dM[c], np.broadcast_to(M0, [nw, 6, 6]))
                assert np.array_equal(dBb[c], np.broadcast_to(B0, [nw, 6, 6]))
                continue
            for got, want in ((dM[c], hM[c]), (dBb[c], hBb[c])):
                bound = 8 * AC.EPS * np.abs(want).max(axis=(1, 2))
                assert np.all(np.abs(got - want).max(axis=(1, 2)) <= bound), (c, per_bin)
    print(f"nw={nw}, ncase={ncase}: device and host header bit-equal: {np.array_equal(dM, hM) and np.array_equal(dBb, hBb)}")


@pytest.mark.parametrize("nw", NWS)
def test_rows_are_independent(launches, nw):
    """Row 0 of the 67-case launch equals the 1-case launch bit for bit, rows 0..2 the 3-case launch."""
    for per_bin in (False, True):
        one, three, many = (launches(nw, n, per_bin) for n in NCASES)
        for k in range(3):
            assert np.array_equal(many[k][:1], one[k])
            assert np.array_equal(many[k][:3], three[k])


def test_entry_refuses_bad_tables_with_a_context(pool):
    """The same refusals with a real context: nothing is launched."""
    pair_case, picks = layout(3, pool)
    loads, dloads, param, modes = tables(pool, picks)
    M0, B0 = bases(5, False)
    with pytest.raises(ValueError, match="decreases"):
        device_mb(3, pair_case[::-1], modes, loads, dloads, param, grid(5), M0, B0)
    with pytest.raises(ValueError, match="aeroServoMod 3"):
        device_mb(3, pair_case, [3, 1, 2], loads, dloads, param, grid(5), M0, B0)
    with pytest.raises(ValueError, match=r"outside \[0, 2\)"):
        device_mb(2, pair_case, modes, loads, dloads, param, grid(5), M0, B0)


# ------------------------------------------------------------------------------ aeroMBBatch against the host path
def fresh(mod, settings=None):
    """A newly built model for each side of a comparison (the rotor keeps its yaw between cases)."""
    import raft
    d = load_design("VolturnUS-S_aero")
    d["turbine"]["aeroServoMod"] = mod
    if settings:
        d.setdefault("settings", {}).update(settings)
    return raft.Model(d)


@pytest.mark.parametrize("grid_name", ["own", "nw200"])
@pytest.mark.parametrize("mod", [1, 2])
def test_aero_mb_batch_against_the_host_path(mod, grid_name):
    """FOWT.aeroMBBatch against calcTurbineConstants(bem=rotorLoadsBatch(...)) plus linear_matrices per
    case, on the design's own grid and on a 200-bin grid (more than one tile): M and B per bin within
    8 eps max|entry| plus the aero term's bar, f_aero0 within 1e-9 of |T| times the lever arm."""
    from raft.prep import linear_matrices
    settings = None if grid_name == "own" else {"min_freq": 0.001, "max_freq": 0.2}
    cases = [dict(c) for c in FIVE]
    a = fresh(mod, settings)
    fa = a.fowtList[0]
    assert grid_name == "own" or fa.nw == 200
    fa.calcTurbineConstants(dict(cases[0], wind_speed=0.0), ptfm_pitch=0)
    out = fa.aeroMBBatch(cases, fa.device_design(), a.device)
    M, B, f0 = (out[k].cpu().numpy() for k in ("M", "B", "f_aero0"))
    assert M.shape == (5, fa.nw, 6, 6) and f0.shape == (5, 6)
    assert not np.any(fa.A_aero) and not np.any(fa.B_aero) and not np.any(fa.B_gyro)     # the host attributes stay
    b = fresh(mod, settings)
    fb = b.fowtList[0]
    bems = fb.rotorLoadsBatch(cases, b.device)
    for i, case in enumerate(cases):
        ref = AC.python_terms(fb, case, bems[i])
        if i == 4:
            assert not np.any(ref["A"]) and not np.any(ref["B"]) and not np.any(f0[i])
            assert np.array_equal(M[i], ref["M_lin"]) and np.array_equal(B[i], ref["B_lin"])
            continue
        for got, want, term in ((M[i], ref["M_lin"], ref["A"]), (B[i], ref["B_lin"], ref["B"])):
            assert np.any(term) or (mod == 1 and term is ref["A"])
            bound = 8 * AC.EPS * np.abs(want).max(axis=(1, 2)) + AERO_TERM_BAR * np.abs(term).max()
            err = np.abs(got - want).max(axis=(1, 2))
            assert np.all(err <= bound), (i, float((err / bound).max()))
        T = abs(fb.rnaList[0].aero_thrust)
        lever = max(1.0, float(np.linalg.norm(fb.rnaList[0].r_hub_rel)))
        assert T > 1e5
        assert np.all(np.abs(f0[i, :3] - ref["f0"][:3]) <= 1e-9 * T)
        assert np.all(np.abs(f0[i, 3:] - ref["f0"][3:]) <= 1e-9 * T * lever)


def test_aero_mb_refuses_a_table_whose_modes_differ():
    """DeviceRotor.aero_mb: the kernel reads the mode from the parameter row, the entry validates the
    host column; rows that disagree with it are a ValueError before any launch."""
    import torch
    from raft import _native as N
    m = fresh(2)
    fowt = m.fowtList[0]
    dr = fowt._device_rotor([0], m.device)
    f64 = dict(dtype=torch.float64, device=dr.device)
    res = dict(loads=torch.zeros([1, 8], **f64), dloads=torch.zeros([1, 2, 3], **f64))
    param = np.zeros([1, N.AP_COUNT])
    param[0, N.AP["MODE"]] = 1
    base = fowt.device_design()
    with pytest.raises(ValueError, match="mode column differs"):
        dr.aero_mb(res, 1, [0], [2], param, base.w, base.M, base.B)


# ------------------------------------------------------------------------------ analyzeCasesBatch
@pytest.fixture(scope="module")
def solved():
    """mod -> analyzeCasesBatch of the five cases with rotor_device=True (the yardstick), solved once."""
    return {mod: fresh(mod).analyzeCasesBatch([dict(c) for c in FIVE], rotor_device=True) for mod in (1, 2)}


@pytest.mark.parametrize("mod", [1, 2])
def test_analyze_cases_batch_with_device_aero(solved, mod):
    """analyzeCasesBatch(aero_device=True) against rotor_device=True: identical drag iteration counts
    and status, the parked case's rows bit-equal, Xi normwise at ten times the measured difference;
    f_aero0 [n, 6] with zeros for the parked case."""
    a = solved[mod]
    m = fresh(mod)
    b = m.analyzeCasesBatch([dict(c) for c in FIVE], aero_device=True)
    assert np.array_equal(a["iters"], b["iters"]) and np.array_equal(a["status"], b["status"])
    for k in ("Xi", "std", "psd"):
        assert np.array_equal(a[k][4], b[k][4])
    worst = max(float(np.linalg.norm(b["Xi"][i] - a["Xi"][i]) / np.linalg.norm(a["Xi"][i])) for i in range(4))
    print(f"analyzeCasesBatch(aero_device=True), aeroServoMod {mod}: Xi normwise difference {worst:.2e}")
    assert worst <= XI_BAR[mod], worst
    assert "f_aero0" not in a and b["f_aero0"].shape == (5, 6)
    assert not np.any(b["f_aero0"][4]) and np.all(b["f_aero0"][:4, 0] > 1e5)
    fowt = m.fowtList[0]
    assert not np.any(fowt.A_aero) and not np.any(fowt.B_aero) and not np.any(fowt.B_gyro)


def test_aero_device_false_is_the_default(solved):
    """Passing aero_device=False explicitly gives the same bits as omitting it."""
    a = solved[2]
    b = fresh(2).analyzeCasesBatch([dict(c) for c in FIVE], rotor_device=True, aero_device=False)
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_no_wind_case_gets_zero_mean_load():
    """Without any operating case the result still carries f_aero0, all zeros."""
    r = fresh(1).analyzeCasesBatch([dict(FIVE[4]), dict(FIVE[4], wave_height=2)], aero_device=True)
    assert r["f_aero0"].shape == (2, 6) and not np.any(r["f_aero0"])

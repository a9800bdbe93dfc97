"""Potential-flow coefficient files (potFirstOrder = 1) on the host: the WAMIT .1 / .3 reader
(raft/bem_io.py), FOWT.readHydro / calcBEM against the reference's interpolated tables
(tests/golden/bem_*.npz, make_bem_golden.py), and the refusals.  No GPU: building a FOWT and its
host tables is NumPy work."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_design, load_golden

BEM = os.path.join(GOLDEN, "bem")
GRID = dict(min_freq=0.02, max_freq=0.4)


def bem_design(hydro, master, first=1, **settings):
    d = load_design("OC3spar")
    d["settings"].update(GRID)
    d["settings"].update(settings)
    d["platform"]["potModMaster"] = master
    if first is not None:
        d["platform"]["potFirstOrder"] = first
    if hydro is not None:
        d["platform"]["hydroPath"] = os.path.join(BEM, hydro)
    return d


def make_fowt(hydro, master, **kw):
    import raft
    return raft.Model(bem_design(hydro, master, **kw)).fowtList[0]


# ---------------------------------------------------------------------------- the reader
def test_reader_buoy_shapes_and_order():
    from raft.bem_io import read_wamit1, read_wamit3
    A, B, w = read_wamit1(os.path.join(BEM, "Buoy.1"), TFlag=True)
    assert A.shape == B.shape == (6, 6, 30) and w.shape == (30,)
    per = np.array([float(f"{0.2 * i:.1f}") for i in range(1, 31)])     # the file's first column, in file order
    np.testing.assert_allclose(w, 2 * np.pi / per, rtol=1e-15)
    assert A[0, 0, 0] == 1.739347E-01 and B[0, 0, 0] == 2.930294E-09        # the file's columns as they are
    assert A[0, 1, 0] == 3.450830E-17 and A[5, 5, 0] == 2.929309E-11
    Mod, Pha, Re, Im, w3, heads = read_wamit3(os.path.join(BEM, "Buoy.3"), TFlag=True)
    assert Mod.shape == Pha.shape == Re.shape == Im.shape == (1, 6, 30)
    assert list(heads) == [0.0]
    np.testing.assert_array_equal(w3, w)
    assert (Mod[0, 0, 0], Pha[0, 0, 0], Re[0, 0, 0], Im[0, 0, 0]) == (1.693418E-03, 9.0E+01, 1.193575E-11, 1.693418E-03)
    w_raw = read_wamit1(os.path.join(BEM, "Buoy.1"), TFlag=False)[2]
    np.testing.assert_array_equal(w_raw, per)                                # without TFlag: the column itself


def test_reader_synthetic_sentinels_and_first_appearance():
    from raft.bem_io import read_wamit1, read_wamit3
    A, B, w = read_wamit1(os.path.join(BEM, "synth.1"), TFlag=True)
    assert A.shape == (6, 6, 12)
    assert w[0] == 0.0 and np.isinf(w[1])                                    # periods -1 and 0
    per = np.array([80.0, 60.0, 45.0, 30.0, 20.0, 12.0, 8.0, 5.0, 3.5, 2.2])
    np.testing.assert_allclose(w[2:], 2 * np.pi / per, rtol=1e-15)            # file order: not sorted
    assert not B[:, :, :2].any() and B[0, 0, 2:].all()                       # four-column rows: B = 0
    assert A[0, 0, 0] != 0 and A[0, 0, 1] != 0
    assert A[0, 1].any() == False and A[2, 5].any() == False                 # noqa: E712  absent entries are zero
    np.testing.assert_array_equal(A, np.swapaxes(A, 0, 1))                   # the generator's symmetric A
    for name, order in (("synth", [0.0, 90.0, 180.0, -90.0]), ("synth_unsorted", [180.0, -90.0, 0.0, 90.0])):
        Mod, Pha, Re, Im, w3, heads = read_wamit3(os.path.join(BEM, name + ".3"), TFlag=True)
        assert list(heads) == order                                          # first appearance, signs kept
        assert Re.shape == (4, 6, 10)
        np.testing.assert_allclose(w3, 2 * np.pi / per, rtol=1e-15)
        np.testing.assert_allclose(Mod, np.hypot(Re, Im), rtol=2e-6)
    s = read_wamit3(os.path.join(BEM, "synth.3"), TFlag=True)
    u = read_wamit3(os.path.join(BEM, "synth_unsorted.3"), TFlag=True)
    np.testing.assert_array_equal(s[2][[2, 3, 0, 1]], u[2])                  # the same rows under another order


def test_reader_rejects_short_rows(tmp_path):
    from raft.bem_io import read_wamit1
    p = tmp_path / "bad.1"
    p.write_text(" 1.0 1 1\n")
    with pytest.raises(ValueError, match="columns"):
        read_wamit1(str(p), TFlag=True)


# ---------------------------------------------------------------------------- the tables
def close(a, b, tol=1e-12):
    return np.max(np.abs(a - b)) <= tol * np.max(np.abs(b))


@pytest.mark.parametrize("tag,hydro,master", [("bem_a", "Buoy", 1), ("bem_b", "synth", 3),
                                              ("bem_c", "synth_unsorted", 3)])
def test_tables_match_reference(tag, hydro, master):
    T = load_golden(tag)
    f = make_fowt(hydro, master)
    np.testing.assert_array_equal(f.w, T["w"])
    if master == 3:
        assert list(f.BEM_headings) == [x % 360 for x in
                                        ([0.0, 90.0, 180.0, -90.0] if hydro == "synth" else [180.0, -90.0, 0.0, 90.0])]
        f.calcBEM()                                    # as analyzeCases: sorted
        assert list(f.BEM_headings) == [0.0, 90.0, 180.0, 270.0]
    np.testing.assert_array_equal(f.BEM_headings, T["BEM_headings"])
    for k in ("A_BEM", "B_BEM", "X_BEM"):
        assert getattr(f, k).shape == T[k].shape
        assert close(getattr(f, k), T[k]), k
    assert f.A_BEM.any() and f.X_BEM.any()


def test_read_hydro_unsorted_tables_of_the_fowt_level_fixture():
    """readHydro's own tables (no calcBEM): file-order headings, each rotated by the file's value."""
    T = load_golden("bem_d")
    f = make_fowt("synth", 0)
    assert f.potMod and f.bem_excitation()
    np.testing.assert_array_equal(f.BEM_headings, T["BEM_headings"])
    for k in ("A_BEM", "B_BEM", "X_BEM"):
        assert close(getattr(f, k), T[k]), k


def test_excitation_switch_follows_the_reference():
    assert not make_fowt("Buoy", 1).bem_excitation()          # potFirstOrder 1 + potModMaster 1: A/B only, no F_BEM
    assert make_fowt("synth", 3).bem_excitation()
    assert make_fowt("synth", 2).bem_excitation()


def test_per_bin_matrices_carry_the_bem_terms():
    from raft.prep import host_tables
    T = load_golden("bem_a")
    f = make_fowt("Buoy", 1)
    f.setStatics({k: T[k] for k in ["M_struc", "B_struc", "C_struc", "C_hydro", "C_moor"]})
    f.setPosition(T["r6"])
    f.calcStatics()
    f.calcHydroConstants()
    h = host_tables(f)
    assert h["per_bin"] is True and "bem" not in h
    off, shape = h["layout"]["M"]
    M = h["packed"][off:off + int(np.prod(shape))].reshape(shape)
    want = np.moveaxis((T["M_struc"][:, :, None] + T["A_BEM"]) + T["A_hydro_morison"][:, :, None], 2, 0)
    assert close(M, want, 1e-13)
    g = make_fowt("synth", 3)
    g.setPosition(np.zeros(6))
    g.calcStatics()
    g.calcHydroConstants()
    hb = host_tables(g)
    assert hb["per_bin"] is True and hb["bem"]["X"].shape == (4, 6, 20)


def test_without_pot_first_order_nothing_changes():
    import raft
    from raft.prep import host_tables
    d = load_design("OC3spar")
    d["settings"].update(GRID)
    f = raft.Model(d).fowtList[0]
    f.setPosition(np.zeros(6))
    f.calcStatics()
    f.calcHydroConstants()
    f.calcBEM()                                               # a no-op for potModMaster 1
    h = host_tables(f)
    assert h["per_bin"] is False and "bem" not in h
    assert f.potFirstOrder == 0 and not f.A_BEM.any() and f.X_BEM is None


# ---------------------------------------------------------------------------- errors
def test_out_of_range_frequency_raises():
    with pytest.raises(ValueError, match="range"):
        make_fowt("synth", 1, max_freq=0.6)                  # 0.6 Hz is above the files' shortest period (2.2 s)


def test_missing_hydro_path_raises_the_reference_text():
    with pytest.raises(Exception, match="If potFirstOrder==1, then hydroPath must be specified in the platform input."):
        make_fowt(None, 1)


def test_pot_mod_master_3_needs_pot_first_order():
    import raft
    m = raft.Model(bem_design("synth", 3, first=None))
    with pytest.raises(ValueError, match="potFirstOrder: 1"):
        m.fowtList[0].calcBEM()
    m.design["cases"] = {"keys": ["wave_heading"], "data": [[0]]}
    with pytest.raises(ValueError, match="potFirstOrder: 1"):
        m.analyzeCases()


@pytest.mark.parametrize("master", [0, 2])
def test_bem_solver_runs_are_refused_by_name(master):
    import raft
    from raft.prep import host_tables
    d = load_design("OC3spar")                                # its spar is a potMod member
    d["settings"].update(GRID)
    d["platform"]["potModMaster"] = master
    m = raft.Model(d)
    f = m.fowtList[0]
    with pytest.raises(NotImplementedError, match="pyHAMS"):
        f.calcBEM()
    with pytest.raises(NotImplementedError, match="pyHAMS"):
        m.analyzeCasesBatch([dict(wave_heading=0, wave_period=10, wave_height=2)])
    f.setPosition(np.zeros(6))
    f.calcStatics()
    f.calcHydroConstants()
    with pytest.raises(NotImplementedError, match="pyHAMS"):  # solveDynamics without calcBEM: no strip-only answer
        host_tables(f)


def test_native_and_light_batches_refuse_coefficient_files():
    from raft.batch import DesignBatch, solve_sweep
    d = bem_design("synth", 3)
    for kw in (dict(native=True), dict(light=True)):
        with pytest.raises(NotImplementedError, match="potFirstOrder"):
            DesignBatch([d], **kw)
    with pytest.raises(NotImplementedError, match="potFirstOrder"):
        solve_sweep([d], None, [0], [0], [dict(wave_heading=0, wave_period=10, wave_height=2)])


def test_nan_in_the_files_is_reported(tmp_path):
    import shutil
    for ext in (".1", ".3"):
        shutil.copy(os.path.join(BEM, "synth" + ext), tmp_path / ("nan" + ext))
    p = tmp_path / "nan.1"
    lines = p.read_text().splitlines()
    cols = lines[80].split()
    cols[3] = "nan"
    lines[80] = " ".join(cols)
    p.write_text("\n".join(lines) + "\n")
    d = bem_design("synth", 1)
    d["platform"]["hydroPath"] = str(tmp_path / "nan")
    import raft
    with pytest.raises(Exception, match="NaN values detected in HAMS calculations for added mass"):
        raft.Model(d)

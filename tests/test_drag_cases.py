"""CPU: the designs, the long-double reference and the criteria of tests/test_gpu_drag.py
(tests/helpers/drag_cases.py) are what they claim to be, and the criteria can be met: the same formulas
in float64 are compared with the reference in the device tests' measure and stay within a quarter of
every bound, and they agree with oracle/raft_oracle.py's hydro_linearization and drag_excitation
driven through the design itself, which ties the long-double formulas to the oracle.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import drag_cases as D   # noqa: E402

from oracle import raft_oracle as O   # noqa: E402

U, LD = D.U, D.LD
_IN = {}


def inputs(name, nw):
    if (name, nw) not in _IN:
        d = D.DragDesign(name, nw)
        _IN[(name, nw)] = (d, D.motions(nw), *D.oracle_inputs(d))
    return _IN[(name, nw)]


def test_long_double_is_wider_than_double():
    assert np.finfo(np.longdouble).eps < 2.0 ** -60


def test_default_design_has_every_branch():
    d = D.DragDesign("default", 33)
    kinds = [c[0] for c in d.comp]
    sizes = [c[1] for c in d.comp]
    assert sorted(kinds) == ["all", "end", "mid", "none", "side"]
    assert 1 in sizes and 2 in sizes and max(sizes) > 64
    rect = ~d.circ
    assert d.circ.sum() == 72 and rect.sum() == 4
    assert np.all(d.area[d.circ, 1] == d.area[d.circ, 2]) and np.all(d.area[d.circ, 0] == np.pi * d.ds[d.circ, 0] * d.dls[d.circ])
    assert np.all(d.area[rect, 1] != d.area[rect, 2]) and np.all(d.Cd_p1[rect] != d.Cd_p2[rect])
    assert np.array_equal(d.area[rect, 0], 2 * (d.ds[rect, 0] + d.ds[rect, 0]) * d.dls[rect])
    ax = d.axial
    for m, (kind, cnt) in enumerate(d.comp):
        a = ax[d.mstart[m]:d.mstart[m + 1]]
        sl = slice(d.mstart[m], d.mstart[m + 1])
        aq, ae = d.area[sl, 0] * d.Cd_q[sl], d.area[sl, 3] * d.Cd_End[sl]
        if kind == "all":
            assert a.all() and (ae != 0).any() and (ae == 0).any()
        elif kind == "none":
            assert not a.any()
            assert ((d.Cd_End[sl] != 0) & (d.area[sl, 3] == 0)).any() and ((d.area[sl, 3] != 0) & (d.Cd_End[sl] == 0)).any()
        elif kind == "mid":
            assert cnt == 3 and list(a) == [False, True, False]
        elif kind == "end":
            assert a.all() and not aq.any() and ae.all()
        elif kind == "side":
            assert a.all() and aq.all() and not ae.any()
    assert len(D.HEADINGS_DEG) >= 2 and D.HEADINGS_DEG[1] != D.HEADINGS_DEG[0]


@pytest.mark.parametrize("name", list(D.DESIGNS))
def test_design_geometry(name):
    d = D.DragDesign(name, 33)
    assert d.nn == int(name[2:]) if name != "default" else d.nn == 76
    assert np.abs(np.linalg.norm(d.rA, axis=1)).max() <= 60.0
    for m in range(d.nm):
        q, p1, p2 = d.mq[m], d.mp1[m], d.mp2[m]
        F = np.stack([q, p1, p2])
        assert np.abs(F @ F.T - np.eye(3)).max() <= 4 * U
        assert np.array_equal(p2, np.cross(q, p1)) and np.linalg.det(F) > 0
        t = d.t[d.mstart[m]:d.mstart[m + 1]]
        assert t[0] == 0 and np.all(np.diff(t) > 0)
    rr = d.rA[d.member].astype(LD) + d.t.astype(LD)[:, None] * d.q.astype(LD)
    assert np.all(np.abs(d.r_rel.astype(LD) - rr).max(axis=1) <= 2 * U * np.linalg.norm(d.r_rel, axis=1))
    assert np.array_equal(d.r, d.r_rel + D.OFFSET) and np.all(d.r[:, 2] < 0)
    h = d.host_tables()
    from raft import _native as N
    off, shape = h["layout"]["memb"]
    memb = h["packed"][off:off + int(np.prod(shape))].reshape(shape)
    assert shape == (N.MF_COUNT, d.nm) and np.array_equal(memb[9:12].T, np.cross(d.rA, d.mp1))
    off, shape = h["layout"]["node"]
    node = h["packed"][off:off + int(np.prod(shape))].reshape(shape)
    assert np.array_equal(node[N.NF["T"]], d.t) and np.array_equal(node[N.NF["AEND"]], d.area[:, 3])
    assert list(h["mstart"]) == list(d.mstart) and h["mstart"][-1] == d.nn


def test_node_counts_lie_on_the_intended_side():
    nm = 5
    for nw in (513, 600, 1000, 1024):
        assert D.solve_kernel(nw, 76, nm) == "2x512" and D.solve_kernel(nw, 77, nm) == "two-pass"
        assert D.solve_kernel(nw, 211, nm) == "two-pass" and D.solve_kernel(nw, 212, nm) == "general"
    for name in ("default", "nn40") + D.SMALL:
        d = D.DragDesign(name, 33)
        assert [D.solve_kernel(nw, d.nn, d.nm) for nw in (33, 97, 200, 257, 513, 1000, 1025)] == \
            ["1x128", "1x128", "2x128", "1x512", "2x512", "2x512", "two-pass"]
    for name, kern in zip(D.LARGE, ("two-pass", "general")):
        d = D.DragDesign(name, 33)
        assert d.nm == nm and D.solve_kernel(600, d.nn, d.nm) == kern
    assert D.DragDesign("nn77", 33).comp[3] == ("all", 70)
    # the edges the small designs sit at: the SER chunking cn = 3 LW nn / 27 at LW = 2 and its 27-entry floor
    assert [3 * 2 * n < 27 for n in (1, 4, 5, 11)] == [True, True, False, False]


SHAPES = [("default", 2), ("default", 33), ("default", 63), ("default", 257), ("default", 1025), ("default", 2048),
          ("nn1", 2), ("nn1", 33), ("nn4", 2), ("nn4", 97), ("nn5", 200), ("nn5", 257), ("nn11", 63), ("nn11", 97),
          ("nn40", 2), ("nn40", 1000), ("nn77", 2), ("nn77", 600), ("nn212", 2), ("nn212", 600)]


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_float64_formulas_against_reference_and_oracle(shape):
    name, nw = shape
    d, Xi, zeta, uhat, finer = inputs(name, nw)
    rng = np.random.default_rng(5)
    for ic, case in enumerate(D.drag_cases()):
        fext = (rng.standard_normal([6, nw]) + 1j * rng.standard_normal([6, nw])) * 1e3 if ic == 0 else None
        ref = D.drag_reference(d, Xi[ic], zeta[ic], uhat, finer, fext)
        f64 = D.drag_reference(d, Xi[ic], zeta[ic], uhat, finer, fext, real=np.float64)
        if ic == D.STILL:
            for a in (ref.sums, ref.Bmat, ref.B_drag, ref.F_drag, ref.F_wave):
                assert np.all(a == 0)
            continue
        # the v_ref floor of the criteria
        assert ref.vfloor.min() >= 1e-3, (shape, ic, ref.vfloor.min())
        bd = D.bounds(ref)
        ratios = {k: D.worst(getattr(f64, k), getattr(ref, k), getattr(bd, k)) for k in ("sums", "Bmat", "B_drag", "F_drag", "F_wave")}
        print(f"float64 vs long double {shape} case {ic}: " + ", ".join(f"{k} {v:.4f}" for k, v in ratios.items()),
              f"; v floor {ref.vfloor.min():.3f}")
        for k, v in ratios.items():
            assert v <= 0.25, (shape, ic, k, v)
        # the oracle itself, on the same inputs
        B, Bm, F = O.hydro_linearization(dict(w=d.w, rho=d.rho_water), d, Xi[ic], zeta[ic] * uhat)
        Fd = O.drag_excitation(d, Bm, zeta[ic] * uhat)
        for k, a, b in (("B_drag", B, f64.B_drag), ("Bmat", Bm, f64.Bmat), ("F_drag", F, f64.F_drag), ("F_drag", Fd, f64.F_drag)):
            assert np.abs(a - b).max() <= 1e-12 * np.abs(a).max(), (shape, ic, k)
        for k, a, b in (("B_drag", B, ref.B_drag), ("Bmat", Bm, ref.Bmat), ("F_drag", F, ref.F_drag)):
            assert float(np.abs(a - b).max()) <= 1e-12 * np.abs(a).max(), (shape, ic, k, "long double")


def test_partial_sums_reference():
    """The bin ranges of the sharded path add up to the whole sums."""
    d, Xi, zeta, uhat, finer = inputs("default", 257)
    ref = D.drag_reference(d, Xi[0], zeta[0], uhat, finer)
    parts = sum(ref.tb[:, :, lo:hi].sum(axis=2) for lo, hi in ((0, 100), (100, 100), (100, 193), (193, 257)))
    assert np.all(np.abs(parts - ref.sums) <= 4 * np.finfo(LD).eps * ref.sums)


@pytest.mark.parametrize("shape", [("default", 63), ("default", 257), ("nn11", 63), ("nn11", 257)], ids=str)
def test_random_bmat_excitation_reference(shape):
    """The excitation of a random Bmat (nine independent entries per node) in float64 stays within a quarter
    of its bound, and is O.drag_excitation's."""
    name, nw = shape
    d, Xi, zeta, uhat, finer = inputs(name, nw)
    Bm = D.random_bmat(d.nn)
    assert not np.allclose(Bm, Bm.transpose(0, 2, 1))
    zero = np.zeros_like(Bm, dtype=LD)
    args = (d, Bm, zero, np.abs(Bm).astype(LD), zeta[0], uhat, finer)
    e, e64 = D.excitation_reference(*args), D.excitation_reference(*args, real=np.float64)
    node = D.C_NODE * (d.nn + 16) * U
    rd = D.worst(e64.F_drag, e.F_drag, node * e.G_abs)
    rw = D.worst(e64.F_wave, e.F_wave, node * (e.G_abs + e.G_lin))
    print(f"random Bmat {shape}, float64 vs long double: F_drag {rd:.4f}, F_wave {rw:.4f}")
    assert rd <= 0.25 and rw <= 0.25
    Fd = O.drag_excitation(d, Bm, zeta[0] * uhat)
    assert np.abs(Fd - e64.F_drag).max() <= 1e-12 * np.abs(Fd).max()

"""CPU: the synthetic QTF cases and their long-double reference (tests/helpers/qtf_cases.py), which
tests/test_gpu_qtf_cases.py holds the device kernels to.

Measured here on 2026-10-21, long double (80-bit) against the float64 oracle oracle/qtf_oracle.py, in
units of u S (u = 2^-53, S the sum of the absolute values of an entry's addends):
  A_orc = 200.1   the largest worst(oracle, ref, S) over the synthetic cases on which the oracle is finite
                  ("coarse", surge, the pair w = 2.054 / 2.170 rad/s at k h = 86 / 96: the (2 k h) u of the
                  hyperbolic ratios formed in double below the k h = 89.4 switch); qtf_cases.A_ORC = 201
  amplification   max S / |ref| over the entries above 1e-6 of their DOF's largest: 1.4e4 ("one_n17");
                  qtf_cases.AMP_CAP = 2e4
  fixtures        c3_qtf n2 = 42: 174.0; qtf_rect design B: 27.2; bound qtf_cases.A_FIX = 600.4
The float64 oracle is finite on every case but "deep" (h = 1000 m, k h up to 689), where the Kim & Yue
sinh((k1 + k2)(z + h)) overflows; the long-double reference is finite there.
"""
import os
import sys

import numpy as np
import pytest

from conftest import load_golden
from oracle import qtf_oracle as Q

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import qtf_cases as C  # noqa: E402
from qtf_rect import RUN_IDS, RUNS, rao_of, rect_tables  # noqa: E402

LD = C.LD


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _oracle(c):
    with np.errstate(all="ignore"):
        return Q.qtf_slender(c.T, c.Xz, c.w2, c.k2, c.beta)[:, :, 0, :]


# ---- the restatement is the oracle --------------------------------------------------------------
def test_long_double_restatement_is_the_oracle_on_c3_n42():
    T = load_golden("c3_qtf")
    ref, S = C.qtf_reference(T, T["out_Xi0"], T["w1_2nd"], T["k1_2nd"], 0.0)
    o = Q.qtf_slender(T, T["out_Xi0"], T["w1_2nd"], T["k1_2nd"], 0.0)[:, :, 0, :]
    a = C.worst(o, ref, S)
    e = _rel(ref.astype(complex), T["out_qtf"][:, :, 0, :])
    print(f"c3 n2=42: worst(oracle) {a:.1f} u S, long double against the stored reference {e:.2e}")
    assert a <= C.A_FIX, a
    assert e < 1e-12, e


@pytest.mark.parametrize("run,ib,moving", RUNS, ids=RUN_IDS)
def test_long_double_restatement_is_the_oracle_on_rect_design_b(run, ib, moving):
    R = load_golden("qtf_rect")
    T = rect_tables(R, "B")
    X, beta = rao_of(R, moving), float(R["qtf_betas"][ib])
    ref, S = C.qtf_reference(T, X, R["qtf_w"], R["qtf_k"], beta)
    o = Q.qtf_slender(T, X, R["qtf_w"], R["qtf_k"], beta)[:, :, 0, :]
    a = C.worst(o, ref, S)
    e = _rel(ref.astype(complex), R[f"B_qtf_{run}"][:, :, 0, :])
    print(f"design B {run}: worst(oracle) {a:.1f} u S, long double against the stored reference {e:.2e}")
    assert a <= C.A_FIX, a
    assert e < 1e-12, e


# ---- the oracle's own distance, and the conditions on the inputs ---------------------------------
def test_oracle_distance_and_input_conditions():
    a_orc, amp = {}, {}
    for name in C.CASES:
        c, ref, S = C.reference(name)
        assert np.all(np.isfinite(ref.view(LD))) and np.all(np.isfinite(S)), name
        o = _oracle(c)
        finite = bool(np.all(np.isfinite(o.view(float))))
        assert finite == (name != "deep"), f"{name}: float64 oracle finite = {finite}"
        if finite:
            a_orc[name] = C.worst(o, ref, S)
        amp[name] = C.amplification(ref, S)
        # every DOF carries weight: its largest entry is at least 1e-6 of its group's
        mx = np.abs(ref).reshape(-1, 6).max(axis=0)
        grp = np.array([mx[:3].max()] * 3 + [mx[3:].max()] * 3)
        assert np.all(mx >= 1e-6 * grp), (name, mx / grp)
        # the second-order potential's denominator does not cancel
        i1, i2 = np.triu_indices(c.n2, 1)
        cond = 0.0
        if len(i1):
            w, k = c.w2.astype(LD), c.k2.astype(LD)
            d1, d2 = C.pot2nd_denominator(w[i1], w[i2], k[i1], k[i2], c.beta, LD(c.depth), LD(C.G))
            cond = float(((np.abs(d1) + np.abs(d2)) / np.abs(d1 - d2)).max())
            assert cond <= 100, (name, cond)
        print(f"{name}: A_orc {a_orc.get(name, float('nan')):.1f}  max S/|ref| {amp[name]:.2e}  "
              f"denominator condition {cond:.1f}  smallest DOF / group {float((mx / grp).min()):.1e}")
    top = max(a_orc, key=a_orc.get)
    print(f"A_orc = {a_orc[top]:.1f} ({top}); amplification cap {max(amp.values()):.2e}")
    assert a_orc[top] <= C.A_ORC, (top, a_orc[top])
    assert a_orc[top] >= 0.5 * C.A_ORC, "qtf_cases.A_ORC is no longer the measured distance"
    assert max(amp.values()) <= C.AMP_CAP, amp
    # "deep": the overflow is the Kim & Yue sinh((k1 + k2)(z + h)) of the oracle
    c = C.case("deep")
    assert 2 * c.k2.max() * c.depth > 709.8 > c.k2.max() * c.depth


# ---- the host tables ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()


@pytest.mark.parametrize("design", list(C.DESIGNS))
def test_native_tables_equal_numpy_tables_on_synthetic_designs(lib, design):
    from raft.hydro_math import wave_numbers
    from raft.qtf import build_tables, native_tables
    for depth in (200.0, 30.0):
        if design == "spar" and depth == 30.0:
            continue
        f = C.make_fowt(design, depth)
        w2 = np.linspace(0.3, 2.0, 7)
        k2 = wave_numbers(w2, depth)
        for hd in (0.0, 30.0, 90.0, 200.0):
            beta = float(np.deg2rad(hd))
            a = build_tables(f, w2, k2, beta)
            _, end, b = native_tables(f, beta)
            for k in ("qnode", "qmemb", "kray", "qmstart", "kstart"):
                np.testing.assert_array_equal(np.asarray(b[k]), np.asarray(a[k]), err_msg=f"{design} {hd} {k}")
            assert (b["rho"], b["g"], b["h"]) == (a["rho"], a["g"], a["h"])
            assert (a["qnode"].shape[1], a["qmemb"].shape[1], a["kray"].shape[1]) == C.EXPECT[design]


# ---- the cases exercise what they claim ---------------------------------------------------------
def _pads(design):
    nq, nmq, nkr = C.EXPECT[design]
    return (-(8 * nq + 3 * nmq + 18)) % 16, (-(2 * nq)) % 16


def test_designs_have_the_sizes_and_k_tails_they_claim():
    assert [_pads(d)[1] for d in ("one", "one8", "one9")] == [14, 0, 14]
    assert [_pads(d)[0] for d in ("tail0", "mix", "tail15")] == [0, 2, 15]
    assert len({_pads(d)[0] for d in C.DESIGNS}) >= 5
    for design in C.DESIGNS:
        f = C.make_fowt(design, 200.0)
        wet = sum(int(np.sum(m.r[:, 2] < 0)) for m in f.memberList)
        nmq = sum(1 for m in f.memberList if not (m.rA[2] > 0 and m.rB[2] > 0))
        assert (wet, nmq) == C.EXPECT[design][:2], design
    one = C.make_fowt("one", 200.0).memberList[0]
    assert one.shape == "circular" and not one.MCF and one.rA[2] * one.rB[2] < 0 and abs(one.q[2]) == 1
    mix = {m.name: m for m in C.make_fowt("mix", 200.0).memberList}
    col, pont, brace, hor, dry = (mix[k] for k in ("col", "pont", "brace", "hor", "dry"))
    # the column: MacCamy-Fuchs, through the surface, Kim & Yue rows of different radii, an inner dls == 0 node
    assert col.MCF and col.rA[2] * col.rB[2] < 0 and np.any(col.dls[1:-1] == 0)
    assert len(set(np.round(col.ds[col.r[:, 2] < 0], 9))) > 2
    # the pontoon: rectangular, inclined, submerged, Ca_p1 != Ca_p2
    assert pont.shape == "rectangular" and pont.r[:, 2].max() < 0 and 0 < abs(pont.q[2]) < 1
    assert np.all(pont.Ca_p1 != pont.Ca_p2)
    # the brace: its top wet strip is partly submerged
    z, dls = brace.r[:, 2], brace.dls
    assert 0 < abs(brace.q[2]) < 1 and np.sum((z < 0) & (z + 0.5 * dls > 0) & (dls > 0)) == 1
    # the horizontal member: its dls == 0 end nodes are wet and carry end volumes
    assert hor.q[2] == 0 and hor.dls[0] == 0 and hor.dls[-1] == 0 and hor.r[0, 2] < 0
    assert hor._end_volume_area(0)[0] > 0 and hor._end_volume_area(hor.ns - 1)[0] > 0
    assert dry.rA[2] > 0 and dry.rB[2] > 0
    # off-axis and asymmetric
    assert all(abs(m.rA[0]) > 0 and abs(m.rA[1]) > 0 for m in (col, pont, brace, hor))


def test_grids_and_environments_are_what_they_claim():
    n2s = sorted(C.case(f"mix_n{n}").n2 for n in (1, 2, 15, 16, 17, 33))
    assert n2s == [1, 2, 15, 16, 17, 33] and all(C.case(n).n2 <= 33 for n in C.CASES)
    assert {round(np.rad2deg(C.case(n).beta)) for n in C.CASES} == {0, 30, 90, 200}
    # thresholds: neighbours bracket k h = 10 and k h = 89.4 by +-1e-3
    c = C.case("thresholds")
    kh = c.k2 * c.depth
    assert c.n2 == 17 and c.depth == 200.0
    for x, w0 in ((10.0, 0.70), (89.4, 2.09)):
        j = int(np.searchsorted(kh, x))
        assert kh[j - 1] < x < kh[j] and abs(c.w2[j] / c.w2[j - 1] - 1 - 2e-3) < 1e-5 and abs(c.w2[j] - w0) < 0.01
        assert 0 < j - 1 and j < c.n2 - 1                      # frequencies on both sides of each switch
    # deep node: |k z| of about 140 at the spar's keel
    c = C.case("deep_node")
    zmin = min(m.r[:, 2].min() for m in c.fowt.memberList)
    assert zmin == -150.0 and c.w2.max() == 3.0 and 135 < c.k2.max() * 150 < 145
    assert C.EXPECT["spar"][2] == 8
    # shallow: k h from about 0.5; deep: k h to about 690
    c = C.case("shallow")
    assert c.depth == 30.0 and 0.45 < c.k2.min() * c.depth < 0.55
    assert max(-m.r[:, 2].min() for m in c.fowt.memberList) < c.depth
    c = C.case("deep")
    assert c.depth == 1000.0 and c.w2.max() == 2.6 and 680 < c.k2.max() * c.depth < 700
    # RAO cases
    c = C.case("mix_n17")
    assert np.all(np.abs(c.Xi0).min(axis=1) > 0) and c.w[0] < c.w2[0] and c.w[-1] > c.w2[-1]
    assert C.case("fixed").Xi0 is None
    c = C.case("coarse")
    assert c.w2[0] < c.w[0] < c.w[-1] < c.w2[-1] and np.diff(c.w)[0] > np.diff(c.w2)[0]
    # unsorted: two frequencies swapped, the same set as mix_n17
    c = C.case("unsorted")
    assert not np.all(np.diff(c.w2) > 0) and np.array_equal(np.sort(c.w2), C.case("mix_n17").w2)
    # every sorted grid is one the MFMA path takes (w and k strictly increasing)
    for n in C.SORTED:
        c = C.case(n)
        assert np.all(np.diff(c.w2) > 0) and np.all(np.diff(c.k2) > 0), n


def test_unsorted_reference_is_the_sorted_one_reindexed():
    """The pair the reference skips (w2 < w1 at i2 > i1) and its mirror are zero with no addend; every
    other entry is the sorted grid's entry of the same two frequencies."""
    c, ref, S = C.reference("unsorted")
    _, ref0, S0 = C.reference("mix_n17")
    p = np.argsort(c.w2)
    inv = np.argsort(p)
    a = ref0[np.ix_(inv, inv)]
    skip = np.zeros([c.n2, c.n2], dtype=bool)
    skip[5, 6] = skip[6, 5] = True
    assert np.all(ref[skip] == 0) and np.all(S[skip] == 0) and np.all(S[~skip] > 0)
    assert np.all(np.abs(ref - a)[~skip] <= 2.0 ** -60 * S[~skip])


def test_fixed_body_diagonal_has_no_second_order_potential():
    """pot2nd is zero at w1 == w2, so the fixed body's diagonal is the remaining incident terms: real up
    to the long-double rounding (the Hermitian fill leaves the diagonal as it is), and not zero."""
    c, ref, S = C.reference("fixed")
    w, k = c.w2.astype(LD), c.k2.astype(LD)
    acc, p = C._pot2nd(w, w, k, k, LD(c.beta), LD(c.depth), np.array([1, 2, -3], dtype=LD), LD(C.G), LD(C.RHO))
    assert np.all(acc == 0) and np.all(p == 0)
    d = np.arange(c.n2)
    assert np.all(np.abs(ref[d, d].imag) <= 2.0 ** -60 * S[d, d])
    assert np.all(np.abs(ref[d, d].real).max(axis=0) > 0)


def test_nq_zero_leaves_the_pinkster_term():
    c, ref, S = C.reference("dry")
    T = dict(c.T, M_struc=np.zeros([6, 6]))
    r0, s0 = C.qtf_reference(T, c.Xi0, c.w2, c.k2, c.beta)
    assert np.all(r0 == 0) and np.all(s0 == 0) and np.all(np.abs(ref).reshape(-1, 6).max(axis=0) > 0)


# ---- the check function ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mix_n17", "one_n16", "deep", "deep_node"])
def test_check_rejects_a_zeroed_negated_or_swapped_column_of_any_dof(name):
    """What the MFMA path once shipped (a wrong yaw column that the normwise bar could not see): the
    long-double result cast to double passes; with one DOF's column zeroed, negated, conjugated or
    swapped with its neighbour it fails, for every DOF, however small that column is."""
    c, ref, S = C.reference(name)
    good = ref.astype(complex)
    assert C.worst(good, ref, S) <= 1.0
    for d in range(6):
        for what, f in (("zeroed", lambda x: 0 * x), ("negated", lambda x: -x), ("conjugated", np.conj),
                        ("scaled by 1 + 1e-9", lambda x: x * (1 + 1e-9))):
            bad = good.copy()
            bad[..., d] = f(bad[..., d])
            if c.n2 == 1 and what == "conjugated":
                continue                                      # a single real diagonal entry
            wd = C.worst_per_dof(bad, ref, S)
            assert wd[d] > C.BAR, (name, d, what, wd[d])
            assert all(wd[e] <= 1.0 for e in range(6) if e != d)
        bad = good.copy()
        e = (d + 1) % 6
        bad[..., [d, e]] = bad[..., [e, d]]
        assert C.worst(bad, ref, S) > C.BAR, (name, d, "swapped")
    nonf = good.copy()
    nonf[0, 0, 5] = np.nan
    assert C.worst(nonf, ref, S) == np.inf

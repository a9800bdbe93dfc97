"""CPU: pin the QTF oracle (oracle/qtf_oracle.py) against the reference's own outputs
(tests/golden/c3_qtf.npz: OC4semi-RAFT_QTF, potSecOrder=1, run in the build container)."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import load_golden
from oracle import qtf_oracle as Q
from oracle import raft_oracle as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from qtf_rect import RUN_IDS, RUNS, rao_of, rect_tables  # noqa: E402


@pytest.fixture(scope="module")
def T():
    return load_golden("c3_qtf")


def _rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def test_oracle_qtf_n42_matches_reference(T):
    q = Q.qtf_slender(T, T["out_Xi0"], T["w1_2nd"], T["k1_2nd"], 0.0)[:, :, 0, :]
    ref = T["out_qtf"][:, :, 0, :]
    assert _rel(q, ref) < 1e-12
    big = np.abs(ref).max()
    np.testing.assert_allclose(q, ref, rtol=1e-11, atol=1e-13 * big)


@pytest.mark.parametrize("key,beta", [("sub400_qtf", 0.0), ("sub400_beta30_qtf", None)])
def test_oracle_qtf_fine_grid_entries(T, key, beta):
    """Entries of the n2=400 grid (df 0.000825 Hz) on a seeded 24-frequency subset, head-on
    and at 30 deg (the degree/radian quirk Q1 of the wave helpers)."""
    b = float(T["sub400_beta30"]) if beta is None else beta
    q = Q.qtf_slender(T, T["out_Xi0"], T["sub400_w"], T["sub400_k"], b)
    assert _rel(q, T[key]) < 1e-12


def test_oracle_qtf_lower_triangle_is_hermitian_fill(T):
    q = Q.qtf_slender(T, T["out_Xi0"], T["w1_2nd"], T["k1_2nd"], 0.0)[:, :, 0, :]
    i, j = np.tril_indices(len(T["w1_2nd"]), -1)
    np.testing.assert_array_equal(q[i, j], np.conj(q[j, i]))


def test_oracle_force_2nd_matches_reference(T):
    fm, f = Q.hydro_force_2nd(T["out_qtf"], T["w1_2nd"], T["w"], T["out_S"][0], float(T["dw"]))
    np.testing.assert_allclose(fm, T["out_Fhydro_2nd_mean"][0], rtol=1e-12, atol=1e-12 * np.abs(fm).max())
    assert _rel(f, T["out_Fhydro_2nd"][0].real) < 1e-12
    assert np.all(T["out_Fhydro_2nd"][0].imag == 0) and np.all(f[:, -1] == 0)


def test_oracle_second_order_solve_matches_reference(T):
    """Full potSecOrder=1 path: first convergence -> RAO -> QTF -> force -> second pass."""
    case = {k: v[0] for k, v in json.loads(str(T["cases_json"]))[0].items()}
    r = O.solve_dynamics(T, case, int(T["nIter"]), float(T["XiStart"]),
                         second_order=dict(w1_2nd=T["w1_2nd"], k1_2nd=T["k1_2nd"]))
    assert list(r["iters_pair"]) == list(T["out_iters_pair"])
    assert _rel(r["Xi"], T["out_Xi"]) < 1e-12
    assert _rel(r["Xi0"], T["out_Xi0"]) < 1e-12


# ---- rectangular and mixed-Ca members (tests/golden/qtf_rect.npz, make_golden.py golden_qtf_rect)
@pytest.fixture(scope="module")
def R():
    return load_golden("qtf_rect")


@pytest.mark.parametrize("run,ib,moving", RUNS, ids=RUN_IDS)
@pytest.mark.parametrize("tag", ["A", "B"])
def test_oracle_qtf_rect_members_matches_reference(R, tag, run, ib, moving):
    """The reference's calcQTF_slenderBody on rectangular strips and ends, Ca_p1 != Ca_p2, a
    rectangular tapered surface-piercing member and Kim & Yue rows beside them (design B), and
    on VolturnUS-S_example as it is (design A): 24 frequencies, six of them past the first-order
    grid (zero-filled RAO), a seeded RAO in all six DOFs at 0 and 30 degrees, the fixed body at
    30 degrees.  The bar of this file."""
    T = rect_tables(R, tag)
    q = Q.qtf_slender(T, rao_of(R, moving), R["qtf_w"], R["qtf_k"], float(R["qtf_betas"][ib]))
    ref = R[f"{tag}_qtf_{run}"]
    assert q.shape == ref.shape
    assert _rel(q, ref) < 1e-12, _rel(q, ref)
    np.testing.assert_allclose(q, ref, rtol=1e-11, atol=1e-13 * np.abs(ref).max())


def test_oracle_second_order_solve_rect_pontoons_matches_reference(R):
    """potSecOrder=1 solve of VolturnUS-S_example (30 degrees, Hs = 2 m, n2 = 17)."""
    T = rect_tables(R, "A")
    case = {k: v[0] for k, v in json.loads(str(R["cases_json"]))[0].items()}
    r = O.solve_dynamics(T, case, int(R["nIter"]), float(R["XiStart"]),
                         second_order=dict(w1_2nd=R["w1_2nd"], k1_2nd=R["k1_2nd"]))
    assert list(r["iters_pair"]) == list(R["out_iters_pair"])
    assert len(R["out_iters_pair"]) == 2
    assert _rel(r["Xi"], R["out_Xi"]) < 1e-12
    assert _rel(r["Xi0"], R["out_Xi0"]) < 1e-12


def test_rect_fixtures_exercise_the_branches_they_claim(R):
    """From the stored tables: what the qtf_rect designs are there for."""
    A, B = rect_tables(R, "A"), rect_tables(R, "B")
    # design A: rectangular submerged members with Ca_p1 != Ca_p2, no MacCamy-Fuchs member
    assert np.any((A["node_circ"] == 0) & (A["node_sub"] == 1) & (A["node_Ca_p1"] != A["node_Ca_p2"]))
    assert not A["member_mcf"].any() and "node_Imat_MCF_sample" not in A
    # design B: the centre column keeps MCF, the rectangular outer columns lose it
    assert list(B["member_mcf"]) == [1] + [0] * (len(B["member_mcf"]) - 1)
    assert list(B["member_circ"][:4]) == [1, 0, 0, 0]
    mem, sub, circ = B["node_member"], B["node_sub"] == 1, B["node_circ"] == 1
    rect_wl = [im for im in range(len(B["member_circ"])) if not B["member_circ"][im]
               and B["node_r"][mem == im][0, 2] * B["node_r"][mem == im][-1, 2] < 0]
    assert rect_wl, "no rectangular member crossing z = 0"
    for im in rect_wl:       # tapered at the waterline, and inclined
        sel = np.nonzero(mem == im)[0]
        iwl = sel[B["node_sub"][sel] == 1][-1]
        assert iwl != sel[-1] and np.any(B["node_ds"][iwl] != B["node_ds"][iwl + 1])
        assert abs(B["node_q"][sel[0], 2]) < 1.0
    assert np.any(~circ & sub & np.any(B["node_drs"] != 0, axis=1) & (B["node_Ca_End"] != 0))
    assert np.any(sub & (B["node_Ca_p1"] != B["node_Ca_p2"]))
    differs = False
    for im in range(len(B["member_circ"])):
        s = np.nonzero((mem == im) & sub)[0]
        if len(s) and (B["node_Ca_p1"][s[0]] != B["node_Ca_p1"][s[-1]] or B["node_Ca_p2"][s[0]] != B["node_Ca_p2"][s[-1]]):
            differs = True
    assert differs, "Ca equal at every member's first and last submerged node"
    # the grid runs past the first-order grid (zero fill of the RAO) and is two tile rows, one partial
    assert len(R["qtf_w"]) == 24 and np.sum(R["qtf_w"] > A["w"][-1]) >= 3
    assert np.array_equal(A["w"], B["w"]) and R["qtf_X"].shape == (6, len(A["w"]))
    # the motion terms dominate the moving body's QTF: the incident-only terms get a run of their own
    for tag in "AB":
        fixed, moving = np.linalg.norm(R[f"{tag}_qtf_b30_fixed"]), np.linalg.norm(R[f"{tag}_qtf_b30"])
        assert 0 < fixed < 0.5 * moving


@pytest.mark.parametrize("tag", ["c3", "q12_b0", "q12_s1"])
def test_oracle_force_2nd_spectrum_matches_reference(tag):
    """interpMode='spectrum' (raft/raft_fowt.py:1760-1784) against the reference method run on
    the fixture QTFs (tests/golden/f2nd_spectrum.npz, make_golden.py golden_f2nd_spectrum)."""
    G = load_golden("f2nd_spectrum")
    src = load_golden("c3_qtf") if tag == "c3" else load_golden("qtf12d")
    qtf = src["out_qtf"] if tag == "c3" else src["qtf"]
    fm, f = Q.hydro_force_2nd_spectrum(qtf, src["w1_2nd"], src["w"], G[f"{tag}_S0"], float(src["dw"]))
    np.testing.assert_allclose(fm, G[f"{tag}_fmean"], rtol=1e-12, atol=1e-12 * np.abs(fm).max())
    assert G[f"{tag}_f"].dtype == complex and f.dtype == complex
    assert _rel(f, G[f"{tag}_f"]) < 1e-12

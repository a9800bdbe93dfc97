"""GPU parity of the slender-body QTF on rectangular and mixed-Ca members against reference
runs (tests/golden/qtf_rect.npz, make_golden.py golden_qtf_rect): the branches of the
reference's pair loop that OC4semi (tests/test_gpu_qtf.py) never enters -- the rectangular
strip and end volumes (raft/raft_fowt.py:1534-1535, :1584), the Rainey term of Ca_p1 != Ca_p2
(:1561-1575) and the waterline force of a rectangular, tapered, surface-piercing member with
the Ca of its last submerged node (:1615-1627).

Design A: VolturnUS-S_example (rectangular submerged pontoons, no Kim & Yue rows).
Design B: VolturnUS-S_rectcols (rectangular tapered inclined outer columns, three-station
pontoons, a MacCamy-Fuchs centre column: Kim & Yue rows beside rectangular members).
Grid: 24 frequencies (two 16-wide tile rows, one partial), six past the first-order grid.

Bar: the project's parity bar, 1e-9 normwise over all entries and elementwise to 1e-9 of the
largest reference entry, that maximum taken separately over the force DOFs (0-2) and the
moment DOFs (3-5): the moments are 20-40 times the forces here."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import load_design, load_golden, statics_of
from oracle import qtf_oracle as Q

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from qtf_rect import DESIGNS, RUN_IDS, RUNS, rao_of, rect_tables  # noqa: E402

pytestmark = pytest.mark.gpu
RTOL = 1e-9


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


@pytest.fixture(scope="module")
def R():
    return load_golden("qtf_rect")


def make(R, tag, platform=None):
    """The product model of design A or B with the reference's statics, at its position."""
    import raft
    T = rect_tables(R, tag)
    d = load_design(DESIGNS[tag])
    d["platform"].update(platform or {})
    m = raft.Model(d, statics=[statics_of(T)])
    f = m.fowtList[0]
    f.setPosition(T["r6"])
    f.calcStatics()
    f.calcHydroConstants()
    return m, f, T


@pytest.fixture(scope="module")
def models(R):
    """One model per design for the whole module (each QTF call below is a whole call)."""
    out = {}
    for tag in DESIGNS:
        m, f, T = make(R, tag)
        f.w1_2nd, f.k1_2nd = R["qtf_w"].copy(), R["qtf_k"].copy()
        f.w2_2nd, f.k2_2nd = f.w1_2nd.copy(), f.k1_2nd.copy()
        out[tag] = (m, f, T)
    return out


def assert_parity(q, ref, what):
    """1e-9 normwise, and elementwise to 1e-9 of the largest force / moment entry."""
    assert q.shape == ref.shape
    e = rel(q, ref)
    ef = np.abs(q[..., :3] - ref[..., :3]).max() / np.abs(ref[..., :3]).max()
    em = np.abs(q[..., 3:] - ref[..., 3:]).max() / np.abs(ref[..., 3:]).max()
    print(f"{what}: normwise {e:.2e}, forces {ef:.2e}, moments {em:.2e} of their largest entry")
    assert e < RTOL, e
    np.testing.assert_allclose(q[..., :3], ref[..., :3], rtol=0, atol=RTOL * np.abs(ref[..., :3]).max())
    np.testing.assert_allclose(q[..., 3:], ref[..., 3:], rtol=0, atol=RTOL * np.abs(ref[..., 3:]).max())


@pytest.mark.parametrize("path", [0, 1], ids=["mfma", "per_pair"])
@pytest.mark.parametrize("run,ib,moving", RUNS, ids=RUN_IDS)
@pytest.mark.parametrize("tag", ["A", "B"])
def test_qtf_matches_reference_run(R, models, tag, run, ib, moving, path):
    """calcQTF_slenderBody on the default (MFMA) path and on the per-pair kernel against the
    reference's QTF: the seeded RAO at 0 and 30 degrees, the fixed body at 30 degrees."""
    from raft import _native as N
    m, f, T = models[tag]
    f.beta = np.array([float(R["qtf_betas"][ib])])
    ctx = N.context(0)
    N.check(N.lib().rh_set_qtf_path(ctx, path), "rh_set_qtf_path")
    try:
        f.calcQTF_slenderBody(0, Xi0=R["qtf_X"] if moving else None)
    finally:
        N.check(N.lib().rh_set_qtf_path(ctx, 0), "rh_set_qtf_path")
    assert f._qtf_qd.order == 1 and f._qtf_qd.nkr == (6 if tag == "B" else 0)
    assert_parity(f.qtf, R[f"{tag}_qtf_{run}"], f"design {tag} {run} path {path}")


def _device_inputs(R, models, ib=1):
    import torch
    from raft.qtf import QtfDevice
    m, f, T = models["B"]
    dd = f.device_design()
    beta = float(R["qtf_betas"][ib])
    M66 = torch.tensor(f.M_struc, dtype=torch.float64, device=dd.device).contiguous()
    new = lambda: QtfDevice(f, R["qtf_w"], R["qtf_k"], beta, 0)     # noqa: E731
    dev = lambda X: torch.tensor(X, dtype=torch.complex128, device=dd.device)   # noqa: E731
    return f, T, dd, beta, M66, new, dev


def test_rect_design_incident_cached_equals_whole_qtf_and_oracle(R, models):
    """Design B, a second RAO with the incident-wave parts kept (Kim & Yue tile sums of the
    centre column, the node bases of rectangular members): the bits of a whole QTF on a fresh
    workspace, and the oracle's QTF of that RAO at the parity bar."""
    f, T, dd, beta, M66, new, dev = _device_inputs(R, models)
    X1 = R["qtf_X"]
    X2 = X1 * 1.3 + 0.1j
    qd = new()
    a1 = qd.qtf(dd.w, dev(X1), M66).cpu().numpy()
    a2 = qd.qtf(dd.w, dev(X2), M66, incident_cached=True).cpu().numpy()
    fresh = new().qtf(dd.w, dev(X2), M66).cpu().numpy()
    np.testing.assert_array_equal(a2, fresh)
    assert not np.array_equal(a1, a2)
    ref = Q.qtf_slender(T, X2, R["qtf_w"], R["qtf_k"], beta)
    assert_parity(a2[:, :, None, :], ref, "design B second RAO, incident parts kept, vs oracle")


def test_rect_design_tile_sharded_equals_whole_qtf(R, models):
    """rh_qtf_slender_rows over 3 simulated ranks + sum + Hermitian fill: the whole QTF's bits."""
    import torch
    f, T, dd, beta, M66, new, dev = _device_inputs(R, models)
    X = dev(R["qtf_X"])
    qd = new()
    whole = qd.qtf(dd.w, X, M66).cpu().numpy()
    acc = torch.zeros([qd.n2, qd.n2, 6], dtype=torch.complex128, device=dd.device)
    for r in range(3):
        part = torch.zeros_like(acc)
        qd.qtf_rows(dd.w, X, M66, part, r, 3)
        acc += part
    qd.hermitian_fill(acc)
    np.testing.assert_array_equal(acc.cpu().numpy(), whole)


@pytest.mark.parametrize("path", [0, 1], ids=["mfma", "per_pair"])
def test_rect_design_qtf_is_hermitian(R, models, path):
    from raft import _native as N
    f, T, dd, beta, M66, new, dev = _device_inputs(R, models)
    ctx = N.context(0)
    N.check(N.lib().rh_set_qtf_path(ctx, path), "rh_set_qtf_path")
    try:
        q = new().qtf(dd.w, dev(R["qtf_X"]), M66).cpu().numpy()
    finally:
        N.check(N.lib().rh_set_qtf_path(ctx, 0), "rh_set_qtf_path")
    i, j = np.tril_indices(q.shape[0], -1)
    assert np.all(np.abs(q[j, i]).max(axis=0) > 0)       # every DOF has an upper triangle
    np.testing.assert_array_equal(q[i, j], np.conj(q[j, i]))


def test_second_order_solve_of_rect_pontoon_design_matches_reference(R):
    """potSecOrder=1 of VolturnUS-S_example (30 degrees, Hs = 2 m, n2 = 17) through
    Model.solveDynamics and through analyzeCasesBatch against the reference's solve: the same
    iteration pair, and Xi, the QTF, the second-order force, the mean drift and the drag
    damping at 1e-9."""
    m, f, T = make(R, "A", platform=json.loads(str(R["sec_platform_json"])))
    np.testing.assert_array_equal(f.w1_2nd, R["w1_2nd"])
    np.testing.assert_array_equal(f.k1_2nd, R["k1_2nd"])
    case = {k: v[0] for k, v in json.loads(str(R["cases_json"]))[0].items()}
    case["wind_speed"] = 0
    pair = list(R["out_iters_pair"])
    assert len(pair) == 2
    mean = R["out_Fhydro_2nd_mean"][0]
    Xi = m.solveDynamics(dict(case))
    assert f.iterations_pair == pair, (f.iterations_pair, pair)
    for what, a, b in (("Xi", Xi, R["out_Xi"]), ("qtf", f.qtf, R["out_qtf"]),
                       ("Fhydro_2nd", f.Fhydro_2nd, R["out_Fhydro_2nd"]),
                       ("B_hydro_drag", f.B_hydro_drag, R["out_B_drag"])):
        print(f"solveDynamics {what}: {rel(a, b):.2e}")
        assert rel(a, b) < RTOL, (what, rel(a, b))
    assert_parity(f.qtf, R["out_qtf"], "solveDynamics qtf")
    np.testing.assert_allclose(f.Fhydro_2nd_mean[0], mean, rtol=RTOL, atol=RTOL * np.abs(mean).max())
    m2, f2, _ = make(R, "A", platform=json.loads(str(R["sec_platform_json"])))
    r = m2.analyzeCasesBatch([dict(case)], want=("psd", "std", "zeta", "B_drag", "Fhydro_2nd"))
    assert list(r["iters_pair"][0]) == pair, (r["iters_pair"][0], pair)
    for what, a, b in (("Xi", r["Xi"][0], R["out_Xi"][0]), ("Fhydro_2nd", r["Fhydro_2nd"][0], R["out_Fhydro_2nd"][0]),
                       ("B_hydro_drag", r["B_drag"][0], R["out_B_drag"])):
        print(f"analyzeCasesBatch {what}: {rel(a, b):.2e}")
        assert rel(a, b) < RTOL, (what, rel(a, b))
    np.testing.assert_allclose(r["f2nd_mean"][0], mean, rtol=RTOL, atol=RTOL * np.abs(mean).max())

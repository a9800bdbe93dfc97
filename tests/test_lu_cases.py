"""CPU: the inputs of tests/test_gpu_lu.py are what they claim to be, and its criteria can be met.

tests/helpers/lu_cases.py builds adversarial 6 x 6 and two-FOWT 12 x 12 systems and lays them out over
the lanes of the solve kernels.  Checked here, without a GPU: the pivot traces cover every (step, row)
pair; layout() gives, for every elimination step, a wave in which no lane exchanges, one in which all
do and one in which odd and even lanes differ; numpy.linalg.solve (the reference's solver) reaches a
backward error of 4 u on every regular family; and the numpy restatements of the device arithmetic
(device_lu6, device_block12) meet the bounds the device tests assert, so those are expected to pass
before anyone runs them.  The restatements are never the expected value on the device.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import lu_cases as L   # noqa: E402

U = L.U
# every grid of tests/test_gpu_lu.py
NWS = [1, 65, 192, 200, 300, 640, 1088]
_CACHE = {}


def pool():
    """The regular 6 x 6 families with one right-hand side each: fam -> (names, A, b)."""
    if "pool" not in _CACHE:
        rng = np.random.default_rng(4)
        out = {}
        for fam, f in L.REGULAR6.items():
            d = f(12)
            A = np.array([d[k] for k in d])
            out[fam] = (list(d), A, L._cplx(rng, len(A), 6))
        _CACHE["pool"] = out
    return _CACHE["pool"]


def pool12():
    if "p12" not in _CACHE:
        _CACHE["p12"] = [L.systems12(192, case) for case in range(3)]
    return _CACHE["p12"]


def test_traces_cover_every_pair():
    names, A, b = pool()["P"]
    seen = set()
    for M, rhs in zip(A, b):
        seen |= set(L.device_lu6(M, rhs)[1])
    assert seen >= set(L.PAIRS), sorted(set(L.PAIRS) - seen)
    # and one matrix per pair exchanges that pair alone (family_P asserts each trace)
    assert sum(n.startswith("pair") for n in names) == 15


@pytest.mark.parametrize("nw", NWS)
@pytest.mark.parametrize("variant", [0, 1])
def test_layout_meets_the_wave_conditions(nw, variant):
    s = L.layout(nw, variant)
    assert s.nw == nw and len(s.kind) == (nw + 63) // 64
    kinds = L.check_layout(s)
    if nw >= 192:        # three full waves: every step has its quiet, its busy and its mixed wave
        assert {"none", "all", "mixed"} <= kinds
    if nw % 64:
        assert s.kind[-1] == "tail"
    if nw >= 64:         # variant 2, the pool alone: every family and every exact pair within one wave
        p = L.layout(nw, 2)
        assert {"P", "T", "S", "C"} <= set(p.fam[:64])
        assert sum(n.startswith("pair") for n in p.name[:64]) == 15


def test_singular_family_is_singular():
    Z = L.family_Z(3)
    assert sorted(Z) == ["rank 5", "zero", "zero column"]
    b = np.ones(6, dtype=complex)
    for name, A in Z.items():
        assert np.all(np.isnan(L.device_lu6(A, b)[0])), name
        assert np.all(np.isfinite(L.device_lu(A, b, raw=True)[0])), name   # what the NaN rule keeps from being stored
        with pytest.raises(np.linalg.LinAlgError):
            np.linalg.solve(A, b)
    s = L.with_singular(L.layout(192), [5, 70, 191])
    assert s.singular.sum() == 3 and list(s.fam[[5, 70, 191]]) == ["Z"] * 3


def test_numpy_reaches_4u_and_the_emulation_meets_the_device_criteria():
    """6 x 6: eta(numpy) <= 4 u on every family; eta(device_lu6) <= 8 max(eta numpy worst, u) per
    system; on family C the forward error <= 64 kappa_inf u."""
    for fam, (names, A, b) in pool().items():
        eta_np = L.backward_errors(A, b, np.array([np.linalg.solve(M, r) for M, r in zip(A, b)]))
        xd = np.array([L.device_lu6(M, r)[0] for M, r in zip(A, b)])
        eta_d = L.backward_errors(A, b, xd)
        print(f"{fam}: n={len(A)} eta numpy {eta_np.max():.2e} emulation {eta_d.max():.2e}")
        assert eta_np.max() <= 4 * U, (fam, eta_np.max())
        assert eta_d.max() <= 8 * max(eta_np.max(), U), (fam, eta_d.max())
        assert np.all(np.isfinite(xd))
        if fam == "C":
            for M, r, x in zip(A, b, xd):
                kinf = np.linalg.cond(M, np.inf)
                assert L.forward_error(M, r, x) <= 64 * kinf * U


def test_block_emulation_meets_the_block_criteria():
    """12 x 12: numpy <= 4 u; device_block12 meets the GEPP criterion on B-P and on B-W with kappa = 1
    and eta <= 8 u kappa_2(A) on B-W; the 12 x 12 elimination (the LDS kernel) meets the GEPP criterion
    on B-W and B-0; B-0 defeats the raw block arithmetic while numpy solves it; B-Z is NaN on both."""
    for case, (Z, K, F, s) in enumerate(pool12()):
        eta_np, worst = L.numpy_eta(s)
        assert np.nanmax(eta_np) <= 4 * U, (case, np.nanmax(eta_np))
        bound = L.gepp_bound(worst)
        for b in range(s.nw):
            xb = L.device_block12(Z[0, b], Z[1, b], K, F[b])[0]
            xg = L.device_lu(s.A[b], F[b])[0]
            fam = s.fam[b]
            if fam == "B-Z":
                assert np.all(np.isnan(xb)) and np.all(np.isnan(xg)), b
                continue
            assert np.all(np.isfinite(xg)), b
            eg = L.backward_error(s.A[b], F[b], xg)
            assert eg <= bound[fam], (case, b, fam, eg)
            if fam == "B-0":
                assert np.all(np.isnan(xb)), b           # the NaN rule: a singular first block
                raw = L.device_block12(Z[0, b], Z[1, b], K, F[b], raw=True)[0]
                xn = np.linalg.solve(s.A[b], F[b])
                assert np.abs(raw - xn).max() / np.abs(xn).max() > 0.1
                continue
            assert np.all(np.isfinite(xb)), b
            eb = L.backward_error(s.A[b], F[b], xb)
            if fam == "B-W":
                assert np.linalg.cond(s.A[b]) <= 1e3
                assert eb <= 8 * U * s.kappaA[b], (b, eb, s.kappaA[b])
            if fam == "B-P" or s.kappaA[b] < 1.5:
                assert eb <= bound[fam], (case, b, fam, eb)
    fams = set().union(*[set(s.fam) for _, _, _, s in pool12()])
    assert fams == {"B-P", "B-W", "B-0", "B-Z"}


def test_block_layout_exchanges_in_both_eliminations():
    """B-P: the first block follows layout variant 0 and the Schur complement variant 1, confirmed on the
    block arithmetic's own traces (the Schur complement is formed in floating point)."""
    Z, K, F, s = pool12()[0]
    la, ls = L.layout(192, 0, 21, only_p=True), L.layout(192, 1, 28, only_p=True)
    ta, ts = L.traces(la), L.traces(ls)
    for b in range(s.nw):
        if s.fam[b] != "B-P":
            continue
        _, o1, o2 = L.device_block12(Z[0, b], Z[1, b], K, F[b])
        assert sorted({k for k, _ in o1}) == list(np.nonzero(ta[b])[0]), b
        assert sorted({k for k, _ in o2}) == list(np.nonzero(ts[b])[0]), b

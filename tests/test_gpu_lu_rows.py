"""GPU: a lane's solve does not depend on its wave mates.

rh::lu_solve<6> (csrc/rh_device.h) enters the exchange of step k with candidate row i for a whole wave
whenever one of its lanes pivots to row i, so which blocks a lane runs depends on the 63 systems beside
it.  The blocks it runs without pivoting there select what it holds; its bits must not move.

  1. rh_system_solve_batch with nf = 1 (k_system_solve_reg<1>), one case: the 720 row orders of one
     strictly dominant complex matrix (the order prescribes the pivot row of every step: at step k the
     row that holds the matrix's row k) and 64 copies of the matrix as it stands, each system with its own
     right-hand side, laid out as bins
       sorted   by first pivot row (waves mostly uniform at step 0);
       shuffled (seeded: every wave mixes rows at every step);
       intruder the 64 unpermuted systems with one permuted system at lane 17, once per first pivot row;
       ragged   130 bins, the last wave with two live lanes (one permuted, one not) and 62 pad lanes.
     Every system's X has the same bits in every layout, and meets the criterion of tests/test_gpu_lu.py:
     eta <= 8 max(worst eta of numpy.linalg.solve on the family, u) with the residual in mpmath.
  2. one wave with the three exactly singular systems of family Z among regular ones: NaN in their rows,
     the neighbours' bits as in the other layouts.
  3. rh_solve_cases on OC3spar (nw = 65, 130, and 577, where rh_set_solver(ctx, 8) is another kernel) with 4
     sea states: the default against rh_set_solver(ctx, 8) bit for bit, and against the general kernel
     (rh_set_solver(ctx, 1); k_solve_cases<2> and <8> keep the chain form of the exchange) within 1e-12
     with equal iteration counts.
"""
import itertools
import os
import sys

import numpy as np
import pytest

from conftest import load_golden
from test_gpu_axial_rows import make_model, random_cases, rel, solver_mode

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import lu_cases as L   # noqa: E402

pytestmark = pytest.mark.gpu
NCOPY = 64
_CACHE = {}


def pool():
    """The 720 row orders of a dominant matrix, then 64 copies of it: (Systems, first pivot row [784],
    numpy's worst eta of family P on them).  Built once, shared, never written."""
    if "pool" not in _CACHE:
        rng = np.random.default_rng(18)
        B = L._dominant(rng)
        perms = list(itertools.permutations(range(6)))
        assert perms[0] == tuple(range(6)) and len(perms) == 720
        A = np.array([B[list(p)] for p in perms] + [B] * NCOPY)
        first = np.array([p.index(0) for p in perms] + [0] * NCOPY)
        n = len(A)
        s = L.Systems(A, L._cplx(rng, n, 6), ["P"] * n, ["".join(map(str, p)) for p in perms] + ["copy"] * NCOPY)
        for i in (1, 100, 719):          # the order prescribes the pivots: step k takes the row holding row k of B
            rows = list(perms[i])
            want = []
            for k in range(6):
                p = rows.index(k)
                if p != k:
                    want.append((k, p))
                    rows[k], rows[p] = rows[p], rows[k]
            assert L.device_lu6(A[i], s.b[i])[1] == want, (perms[i], want)
        s.eta_np, worst = L.numpy_eta(s)
        _CACHE["pool"] = (s, first, worst)
    return _CACHE["pool"]


def solve_bins(A, b):
    """k_system_solve_reg<1> on the bins A [nw][6][6], b [nw][6]: X [nw][6]."""
    import torch
    from raft import _native as N
    dev = torch.device("cuda", 0)
    nw = len(A)
    Z = torch.tensor(np.ascontiguousarray(A.reshape(1, 1, nw, 36)), device=dev)
    F = torch.tensor(np.ascontiguousarray(b.T[None]), device=dev)
    X = torch.ones([1, 6, nw], dtype=torch.complex128, device=dev)
    N.check(N.lib().rh_system_solve_batch(N.context(0), 1, 1, nw, N.ptr(Z), None, N.ptr(F), N.ptr(X),
                                          N.stream_handle(torch, dev)), "rh_system_solve_batch")
    return np.ascontiguousarray(X.cpu().numpy()[0].T)


def layouts():
    """{name: system index of every bin}"""
    s, first, _ = pool()
    n = s.nw
    out = {"sorted": np.argsort(first, kind="stable"), "shuffled": np.random.default_rng(7).permutation(n)}
    for r in range(1, 6):                # an intruder that pivots to row r at step 0 and goes on exchanging
        cand = [i for i in range(720) if first[i] == r and len(L.device_lu6(s.A[i], s.b[i])[1]) >= 4]
        idx = np.arange(720, 720 + NCOPY)
        idx[17] = cand[0]
        out[f"intruder {r}"] = idx
    rag = out["shuffled"][:130].copy()
    rag[128], rag[129] = 345, 720 + 3    # the last wave: one permuted system, one copy, 62 pad lanes
    assert first[345] != 0
    out["ragged"] = rag
    return out


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def solved():
    """{layout: (bin -> system, X [nw][6])}: every layout solved once, shared by the tests below."""
    if "solved" not in _CACHE:
        s, _, _ = pool()
        _CACHE["solved"] = {name: (idx, solve_bins(s.A[idx], s.b[idx])) for name, idx in layouts().items()}
    return _CACHE["solved"]


def test_layout_covers_every_system_and_mixes_waves():
    s, first, _ = pool()
    lay = layouts()
    assert sorted(lay["sorted"]) == list(range(s.nw)) and sorted(lay["shuffled"]) == list(range(s.nw))
    w = first[lay["sorted"]][:768].reshape(12, 64)
    assert sum(len(set(r)) == 1 for r in w) >= 6           # mostly uniform waves
    w = first[lay["shuffled"]][:768].reshape(12, 64)
    assert all(len(set(r)) >= 4 for r in w)                # every wave mixes rows
    assert len(lay["ragged"]) == 130 and all(len(lay[f"intruder {r}"]) == 64 for r in range(1, 6))


def test_same_bits_in_every_layout():
    s, _, _ = pool()
    res = solved()
    ref = np.zeros([s.nw, 6], dtype=complex)
    idx, X = res["sorted"]
    ref[idx] = X
    assert np.all(np.isfinite(ref))
    for name, (idx, X) in res.items():
        bad = np.nonzero((bits(X) != bits(ref[idx])).any(axis=1))[0]
        assert len(bad) == 0, (name, [(int(b), s.name[idx[b]]) for b in bad[:8]])


def test_every_system_meets_the_gepp_criterion():
    s, _, worst = pool()
    bound = L.gepp_bound(worst)["P"]
    idx, X = solved()["shuffled"]
    eta = L.backward_errors(s.A[idx], s.b[idx], X)
    print(f"k_system_solve_reg<1>: worst eta {eta.max():.2e}, numpy {worst['P']:.2e}, bound {bound:.2e}")
    assert np.all(eta <= bound), (int(np.argmax(eta)), eta.max(), bound)
    for name, (idx, X) in solved().items():      # the small layouts too (the same bits, so the same eta)
        if name.startswith("intruder") or name == "ragged":
            e = L.backward_errors(s.A[idx[[17, -2, -1]]], s.b[idx[[17, -2, -1]]], X[[17, -2, -1]])
            assert np.all(e <= bound), (name, e, bound)


def test_singular_lanes_among_regular_ones():
    s, _, _ = pool()
    ref_idx, ref_X = solved()["sorted"]
    ref = np.zeros([s.nw, 6], dtype=complex)
    ref[ref_idx] = ref_X
    idx = np.random.default_rng(9).permutation(s.nw)[:64]
    A, b = s.A[idx].copy(), s.b[idx].copy()
    Z = L.family_Z(3)
    at = {5: "zero", 40: "zero column", 63: "rank 5"}
    for lane, k in at.items():
        A[lane] = Z[k]
    X = solve_bins(A, b)
    sing = np.zeros(64, dtype=bool)
    sing[list(at)] = True
    assert np.all(np.isnan(X[sing].real)) and np.all(np.isnan(X[sing].imag)), X[sing]
    assert np.array_equal(bits(X[~sing]), bits(ref[idx[~sing]]))


@pytest.mark.parametrize("nw", [65, 130, 577])
def test_solve_cases_default_split_and_general(nw):
    m, f = make_model("OC3spar", load_golden("c1_OC3spar"), {"min_freq": 0.4 / nw})
    assert m.nw == nw
    cases = random_cases(4, 18)
    want = ("psd", "std", "zeta", "rao")
    a = m.analyzeCasesBatch(cases, want=want)
    with solver_mode(8):
        b = m.analyzeCasesBatch(cases, want=want)
    with solver_mode(1):
        c = m.analyzeCasesBatch(cases, want=want)
    assert np.all(np.isfinite(a["Xi"].view(np.float64)))
    for k in ("Xi", "psd", "rao", "std", "zeta", "iters", "status"):
        assert np.array_equal(bits(a[k]) if a[k].dtype.kind in "fc" else a[k],
                              bits(b[k]) if b[k].dtype.kind in "fc" else b[k]), k
    np.testing.assert_array_equal(a["iters"], c["iters"])
    np.testing.assert_array_equal(a["status"], c["status"])
    for ic in range(len(cases)):
        print(nw, ic, int(a["iters"][ic]), rel(a["Xi"][ic], c["Xi"][ic]))
        assert rel(a["Xi"][ic], c["Xi"][ic]) < 1e-12, ic

"""GPU: the slender-body QTF kernels (k_qtf_tables, k_qtf_lk, k_qtf_gemm and the Kim & Yue tile sums of
the MFMA path; k_qtf_pairs, the per-pair kernel) on the synthetic cases of tests/helpers/qtf_cases.py,
entry by entry against the long-double reference: worst(device, ref, S) = max |x - ref| / (u S) over all
pairs and all six DOFs, u = 2^-53, S the sum of the absolute values of an entry's addends.

Bar: qtf_cases.BAR = 8 max(A_orc, 4) = 1608 u S, with A_orc = 201 the float64 oracle's own measured
distance from the long-double reference over all cases (tests/test_qtf_cases.py); each case is held to the
same formula with the oracle's distance on that case alone (qtf_cases.bar: 32 to 1608 u S, about 240 on the
moving-body "mix" cases), and "deep", where the float64 oracle is not finite, to BAR.  The factor 8: the
device sums up to K = 8 nq + 3 nmq + 18 (about 230 here) products per entry in GEMM order and forms the hyperbolic ratios
from exponentials, whose relative error grows with |k z| u.  The bar is tied to the float64
formulation's distance, never to the device's output.

Measured on an MI355X, 2026-10-21, on this kernel source (largest worst over the cases, in u S): MFMA path
210.3, per-pair kernel 198.1, both on "coarse" in surge (the float64 oracle: 200.1 there); "fixed" 82.0 / 82.8;
"deep" 22.4 / 133.3; every other case below 57 (MFMA below 16), each within a quarter of its own bar.  The stated
range of DESIGN.md, "Accuracy of the slender-body QTF" ((k1 + k2) h <= 709.78 with Kim & Yue rows), is what
"deep" asserts.  Before k_qtf_pairs took the per-frequency factors kayt[6] for the Kim & Yue interval factor,
its joint denominator sqrt sqrt cosh(k1 h) cosh(k2 h) overflowed just below that limit and the pair
k h = 167 / 542 of "deep" came out finite and wrong (6.1e13 u S in sway).

The references are computed once per process (qtf_cases.reference) and the device outputs once per
(case, path); every test is a handful of launches on n2 <= 33.
"""
import contextlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import qtf_cases as C  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = complex(-7.25, 3.5)


@contextlib.contextmanager
def _path(path):
    from raft import _native as N
    ctx = N.context(0)
    N.check(N.lib().rh_set_qtf_path(ctx, path), "rh_set_qtf_path")
    try:
        yield
    finally:
        N.check(N.lib().rh_set_qtf_path(ctx, 0), "rh_set_qtf_path")


@contextlib.contextmanager
def _stop_on_device_error():
    """A HIP error (the library's RH_EHIP, or one torch reports) ends the session: nothing more is started
    on a device that has faulted.  Any other error, a refusal of the library included, fails its test."""
    from raft._native import NativeError
    try:
        yield
    except RuntimeError as e:
        if isinstance(e, NativeError) or "hip" in str(e).lower():
            pytest.exit(f"device error, stopping: {e}", returncode=3)
        raise


def _dev(c, X=None):
    import torch
    d = torch.device("cuda", 0)
    return (torch.tensor(c.w, dtype=torch.float64, device=d),
            torch.tensor(c.Xz if X is None else X, dtype=torch.complex128, device=d),
            torch.tensor(c.M, dtype=torch.float64, device=d).contiguous())


def _new(c):
    from raft.qtf import QtfDevice
    qd = QtfDevice(c.fowt, c.w2, c.k2, c.beta, 0)
    assert (qd.nq, qd.nmq, qd.nkr) == C.EXPECT[c.design], (c.name, qd.nq, qd.nmq, qd.nkr)
    assert qd.order == int(c.name != "unsorted")
    return qd


_OUT = {}


def _out(name, path):
    """The whole QTF of a case on a fresh device workspace, path 0 (MFMA) or 1 (per pair): once."""
    if (name, path) not in _OUT:
        c, ref, S = C.reference(name)
        with _stop_on_device_error(), _path(path):
            w, X, M = _dev(c)
            _OUT[name, path] = _new(c).qtf(w, X, M).cpu().numpy()
    return _OUT[name, path]


def _in_range(name, x, ref, S):
    """The entries of the pairs within the device's stated range (all of them but on "deep"), after checking
    that exactly the pairs beyond it are non-finite, in every DOF: never a wrong finite number."""
    c = C.reference(name)[0]
    out = C.beyond_range(c)
    fin = np.isfinite(x.view(float).reshape(c.n2, c.n2, 6, 2)).all(axis=3)
    if out.any():
        print(f"{name}: {int(out.sum())} of {out.size} pairs beyond (k1 + k2) h = 709.78; non-finite entries "
              f"per DOF {[int((~fin[..., d]).sum()) for d in range(6)]}")
    assert out.any() == (name == "deep")
    np.testing.assert_array_equal(fin, np.broadcast_to(~out[:, :, None], fin.shape), err_msg=f"{name}: finite entries")
    return x[~out], ref[~out], S[~out]


def _report(what, x, ref, S, bar):
    wd = C.worst_per_dof(x, ref, S)
    print(f"{what}: worst per DOF " + " ".join(f"{v:.1f}" for v in wd) + f"  (bar {bar:.0f} u S)")
    return max(wd)


@pytest.mark.parametrize("name", C.SORTED)
def test_mfma_path_against_long_double(name):
    """The default path through QtfDevice.qtf on every case with a sorted grid.  On a sorted grid the
    lower triangle is the exact conjugate of the upper.  "fixed" shows the zero diagonal of the
    second-order potential, "dry" (nq = 0, which rh_qtf_slender accepts: its node loops and the
    potential GEMM are empty, K = 18 + 14 zero rows) the Pinkster term alone.  On "deep" (h = 1000 m) the
    pairs with (k1 + k2) h > 709.78 are non-finite in every DOF, as DESIGN.md states (the Kim & Yue
    exp(k1 (z + h)) exp(k2 (z + h)) overflows where the reference's sinh((k1 + k2)(z + h)) does); every
    other pair of that case, k h up to 689, meets the bar against long double.  Both paths alike."""
    c, ref, S = C.reference(name)
    x = _out(name, 0)
    assert x.shape == (c.n2, c.n2, 6)
    worst = _report(f"mfma {name}", *_in_range(name, x, ref, S), C.bar(name))
    assert worst <= C.bar(name), (name, worst)
    i, j = np.tril_indices(c.n2, -1)
    keep = ~C.beyond_range(c)[i, j]
    np.testing.assert_array_equal(x[i, j][keep], np.conj(x[j, i])[keep])


@pytest.mark.parametrize("name", list(C.CASES))
def test_per_pair_kernel_against_long_double(name):
    """rh_set_qtf_path(ctx, 1) on every case; on "unsorted" (order == 0) it is the only path, and the
    pair the reference skips and its mirror are exactly zero (S == 0 there)."""
    c, ref, S = C.reference(name)
    x = _out(name, 1)
    worst = _report(f"per pair {name}", *_in_range(name, x, ref, S), C.bar(name))
    assert worst <= C.bar(name), (name, worst)
    if name == "unsorted":
        np.testing.assert_array_equal(x, _out(name, 0))          # path 0 on order == 0 is the same kernel
        assert not np.any(x[5, 6]) and not np.any(x[6, 5])


@pytest.mark.parametrize("name", C.SORTED)
def test_the_two_paths_agree_elementwise(name):
    c, ref, S = C.reference(name)
    a, _, _ = _in_range(name, _out(name, 0), ref, S)
    b, ref, S = _in_range(name, _out(name, 1), ref, S)
    d = np.abs(a.astype(C.CLD) - b.astype(C.CLD))
    tol = 2 * C.bar(name) * C.LD(C.U) * S
    print(f"paths {name}: largest |a - b| / (u S) {float((d[S > 0] / (C.LD(C.U) * S[S > 0])).max()):.1f}")
    assert np.all(d <= tol), (name, float((d[S > 0] / tol[S > 0]).max()))


@pytest.mark.parametrize("nrank", [1, 3, 8])
@pytest.mark.parametrize("name", ["mix_n15", "mix_n17", "mix_n33"])
def test_sharded_rows_sum_to_the_whole_calls_bits(name, nrank):
    """qtf_rows of every rank into a buffer of sentinels: a rank writes the pairs of its own tiles and
    nothing else (a rank without tiles nothing at all); the parts' sum, Hermitian-filled, is the whole
    call's bits.  n2 = 15: one tile; 17 and 33: 3 and 6 tiles."""
    import torch
    from raft.parallel import qtf_pair_flat, qtf_tiles
    c, ref, S = C.reference(name)
    whole = _out(name, 0)
    n2 = c.n2
    assert -(-n2 // 16) * (-(-n2 // 16) + 1) // 2 == {15: 1, 17: 3, 33: 6}[n2]
    with _stop_on_device_error():
        w, X, M = _dev(c)
        qd = _new(c)
        acc = torch.zeros([n2, n2, 6], dtype=torch.complex128, device=w.device)
        empty = 0
        for r in range(nrank):
            part = torch.full([n2, n2, 6], SENTINEL, dtype=torch.complex128, device=w.device)
            qd.qtf_rows(w, X, M, part, r, nrank)
            wrote = (part != SENTINEL).any(dim=2).cpu().numpy()
            mine = np.zeros(n2 * n2, dtype=bool)
            mine[qtf_pair_flat(n2, qtf_tiles(n2, r, nrank))] = True
            np.testing.assert_array_equal(wrote, mine.reshape(n2, n2), err_msg=f"rank {r} of {nrank}")
            empty += int(not mine.any())
            acc += torch.where(part == SENTINEL, torch.zeros_like(part), part)
        qd.hermitian_fill(acc)
        got = acc.cpu().numpy()
    assert empty >= nrank - {15: 1, 17: 3, 33: 6}[n2] and (n2 != 15 or empty == nrank - 1)
    np.testing.assert_array_equal(got, whole)


@pytest.mark.parametrize("name", C.CACHED)
def test_kept_incident_parts_equal_a_whole_call_and_meet_the_bar(name):
    """A second RAO with incident_cached=True on "mix" and the K-tail designs: the bits of a whole call
    on a fresh workspace, and the long-double bar."""
    c2, ref2, S2 = C.reference(name, seed=1)
    c = C.reference(name)[0]
    assert not np.array_equal(c.Xi0, c2.Xi0)
    with _stop_on_device_error():
        w, X1, M = _dev(c)
        X2 = _dev(c2)[1]
        qd = _new(c)
        a1 = qd.qtf(w, X1, M).cpu().numpy()
        a2 = qd.qtf(w, X2, M, incident_cached=True).cpu().numpy()
        fresh = _new(c2).qtf(w, X2, M).cpu().numpy()
    np.testing.assert_array_equal(a1, _out(name, 0))
    np.testing.assert_array_equal(a2, fresh)
    assert not np.array_equal(a1, a2)
    worst = _report(f"kept incident parts {name}", a2, ref2, S2, C.bar(name, 1))
    assert worst <= C.bar(name, 1), (name, worst)


@pytest.mark.parametrize("path", [0, 1], ids=["mfma", "per_pair"])
@pytest.mark.parametrize("name", ["mix_n1", "mix_n15", "mix_n17"])
def test_nothing_is_written_outside_the_output(name, path):
    """The n2 x n2 x 6 output inside a larger buffer of sentinels (n2 = 1, 15, 17: below a tile, and one
    past it): the sentinels before and after it are untouched, and the output is the usual bits."""
    import torch
    c, ref, S = C.reference(name)
    n, guard = c.n2 * c.n2 * 6, 4096
    with _stop_on_device_error(), _path(path):
        w, X, M = _dev(c)
        buf = torch.full([guard + n + guard], SENTINEL, dtype=torch.complex128, device=w.device)
        out = buf[guard:guard + n].view(c.n2, c.n2, 6)
        _new(c).qtf(w, X, M, out=out)
        got = buf.cpu().numpy()
    assert np.all(got[:guard] == SENTINEL) and np.all(got[guard + n:] == SENTINEL)
    np.testing.assert_array_equal(got[guard:guard + n].reshape(c.n2, c.n2, 6), _out(name, path))

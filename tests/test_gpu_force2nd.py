"""GPU: the second-order force kernels (k_force2nd, k_force2nd_batch, k_force2nd_spec,
k_force2nd_spec_out) and the Hermitian fill (k_qtf_fill) against long-double references, on grid pairs
that aim at the cell search and the interpolation.

Grid pairs, inputs, references and criteria are tests/helpers/force2nd_cases.py (checked on the CPU by
tests/test_force2nd_cases.py): probes bitwise on the first, on inner and on the last QTF frequency with
w running past both ends (searchsorted's side, the clipping, zero strictly outside); nw = 300 > 256 (the
strided loop); n2 = 2 with nw = 2 and 40; w wholly inside w2 (no zeros); w2 disjoint from w (every
value exactly 0.0).  The QTF is random and not Hermitian, so the y/x orientation shows.

Criteria (u = 2^-53): f within (nw + 32) u |ref| per element with the reference's zero pattern and an
exactly zero last bin; f_mean within (nw + 32) u 2 dw sum |S0_i Re Q_ii|; the batched form equal to the
single one bit for bit in its real part with an exactly zero imaginary part, and NaN in every row of a
case whose qidx is outside [0, nq); spectrum mode: Sf within (n2 + 32) u |ref| with Sf[d][0] = 0, f
within (n2 + 36) u |ref|.  The worst ratio to each bound is printed (pytest -s).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import force2nd_cases as F2   # noqa: E402

pytestmark = pytest.mark.gpu
U, LD = F2.U, F2.LD


def dev():
    import torch
    return torch.device("cuda", 0)


def tens(a, dtype=None):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=dev())


def single(x, iq, isp):
    """rh_force_2nd of QTF iq and spectrum isp: (f_mean [6], f [6][nw]) on the host."""
    import torch
    from raft import _native as N
    f = torch.full([6, x.nw], -1.0, dtype=torch.float64, device=dev())
    fm = torch.full([6], -1.0, dtype=torch.float64, device=dev())
    w2, Q, w, S = tens(x.w2), tens(x.Q[iq]), tens(x.w), tens(x.S[isp])
    N.check(N.lib().rh_force_2nd(N.context(0), x.n2, N.ptr(w2), N.ptr(Q), x.nw, N.ptr(w), x.dw, N.ptr(S), N.ptr(f), N.ptr(fm),
                                 N.stream_handle(torch, dev())), "rh_force_2nd")
    torch.cuda.synchronize()
    return fm.cpu().numpy(), f.cpu().numpy()


def batch(x, qidx, nq=2):
    """rh_force_2nd_batch of every spectrum of x: (f_mean [ncase][6], f [ncase][6][nw] complex)."""
    import torch
    from raft import _native as N
    nc = len(x.S)
    f = torch.full([nc, 6, x.nw], complex(-1.0, -1.0), dtype=torch.complex128, device=dev())
    fm = torch.full([nc, 6], -1.0, dtype=torch.float64, device=dev())
    qi = None if qidx is None else tens(np.asarray(qidx), torch.int32)
    w2, Q, w, S = tens(x.w2), tens(x.Q[:nq]), tens(x.w), tens(x.S)
    N.check(N.lib().rh_force_2nd_batch(N.context(0), nc, x.n2, N.ptr(w2), N.ptr(Q), nq, N.ptr(qi), x.nw, N.ptr(w), x.dw,
                                       N.ptr(S), N.ptr(f), N.ptr(fm), N.stream_handle(torch, dev())), "rh_force_2nd_batch")
    torch.cuda.synchronize()
    return fm.cpu().numpy(), f.cpu().numpy()


@pytest.mark.parametrize("name", list(F2.pairs()))
def test_force_2nd_against_long_double(name):
    x = F2.inputs(name)
    for iq, isp in ((0, 0), (1, 1)):
        fm_ref, f_ref, fm_scale = F2.force_reference(x.Q[iq], x.w2, x.w, x.S[isp], x.dw)
        fm, f = single(x, iq, isp)
        assert np.all(np.isfinite(f)) and np.all(np.isfinite(fm))
        rf, rm = F2.force_ratios(f"rh_force_2nd pair {name}", x.nw, fm_ref, f_ref, fm_scale, fm, f)
        print(f"rh_force_2nd pair {name} (n2={x.n2}, nw={x.nw}) QTF {iq}: worst ratio to the bound: f {rf:.3f}, "
              f"f_mean {rm:.3f}; {int((f_ref != 0).sum())} of {f_ref.size} bins non-zero")
        assert rf <= 1.0 and rm <= 1.0, (name, iq, rf, rm)
        if name == "5":
            assert not f.any() and not fm.any()


@pytest.mark.parametrize("name", ["1", "2"])
def test_force_2nd_batch_bit_equal_to_single(name):
    x = F2.inputs(name)
    for qidx in ([1, 0, 1], None):
        fm, f = batch(x, qidx)
        assert not f.imag.any(), "imaginary part"
        for c in range(3):
            fm1, f1 = single(x, 0 if qidx is None else qidx[c], c)
            assert np.array_equal(f[c].real.view(np.int64), f1.view(np.int64)), (name, qidx, c)
            assert np.array_equal(fm[c].view(np.int64), fm1.view(np.int64)), (name, qidx, c)


@pytest.mark.parametrize("name", ["1", "2"])
def test_force_2nd_batch_bad_index_gives_nan(name):
    x = F2.inputs(name)
    fm, f = batch(x, [0, -1, 2])
    for c in (1, 2):
        assert np.all(np.isnan(f[c].real)) and np.all(np.isnan(f[c].imag)) and np.all(np.isnan(fm[c])), c
    fm1, f1 = single(x, 0, 0)
    assert np.array_equal(f[0].real.view(np.int64), f1.view(np.int64)) and not f[0].imag.any()
    assert np.array_equal(fm[0].view(np.int64), fm1.view(np.int64))


@pytest.mark.parametrize("name", F2.SPECTRUM_PAIRS)
def test_force_2nd_spectrum_against_long_double(name):
    import torch
    from raft import _native as N
    x = F2.inputs(name)
    fm_ref, f_ref, Sf_ref, fm_scale = F2.spectrum_reference(x.Q[0], x.w2, x.w, x.S[0], x.dw)
    f = torch.full([6, x.nw], -1.0, dtype=torch.float64, device=dev())
    fm = torch.full([6], -1.0, dtype=torch.float64, device=dev())
    Sf = torch.full([6, x.n2], -1.0, dtype=torch.float64, device=dev())
    w2, Q, w, S = tens(x.w2), tens(x.Q[0]), tens(x.w), tens(x.S[0])
    N.check(N.lib().rh_force_2nd_spectrum(N.context(0), x.n2, N.ptr(w2), N.ptr(Q), x.nw, N.ptr(w), x.dw, N.ptr(S), N.ptr(Sf),
                                          N.ptr(f), N.ptr(fm), N.stream_handle(torch, dev())), "rh_force_2nd_spectrum")
    torch.cuda.synchronize()
    f, fm, Sf = f.cpu().numpy(), fm.cpu().numpy(), Sf.cpu().numpy()
    assert np.all(Sf[:, 0] == 0)
    assert np.array_equal(Sf == 0, Sf_ref == 0), "zero pattern of Sf"
    nz = Sf_ref != 0
    rS = float((np.abs(Sf.astype(LD) - Sf_ref)[nz] / ((x.n2 + 32) * U * Sf_ref[nz])).max()) if nz.any() else 0.0
    rf, rm = F2.force_ratios(f"rh_force_2nd_spectrum pair {name}", x.n2, fm_ref, f_ref, fm_scale, fm, f, extra=4)
    print(f"rh_force_2nd_spectrum pair {name} (n2={x.n2}, nw={x.nw}): worst ratio to the bound: Sf {rS:.3f}, f {rf:.3f}, "
          f"f_mean {rm:.3f}")
    assert rS <= 1.0 and rf <= 1.0 and rm <= 1.0, (name, rS, rf, rm)


@pytest.mark.parametrize("n2", [1, 16, 17, 43])
def test_hermitian_fill(n2):
    """The upper triangle and the diagonal bit-unchanged, the lower triangle exactly conj of the upper."""
    import torch
    from raft import _native as N
    rng = np.random.default_rng(n2)
    Q = rng.standard_normal([n2, n2, 6]) + 1j * rng.standard_normal([n2, n2, 6])
    Qt = tens(Q)
    N.check(N.lib().rh_qtf_hermitian_fill(N.context(0), n2, N.ptr(Qt), N.stream_handle(torch, dev())), "rh_qtf_hermitian_fill")
    torch.cuda.synchronize()
    out = Qt.cpu().numpy()
    iu = np.triu_indices(n2)
    il = np.tril_indices(n2, -1)
    assert np.array_equal(out[iu].view(np.int64), Q[iu].view(np.int64))
    want = np.conj(np.swapaxes(Q, 0, 1))
    assert np.array_equal(out[il].view(np.int64), want[il].view(np.int64))
